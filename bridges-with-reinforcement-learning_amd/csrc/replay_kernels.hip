// K8: prioritised replay on the device (robotoddler/training/records.py, ReplayRing.sample_prioritized / update_priorities):
// the inverse-CDF draw over the priority column of the ring, the write-back of refreshed priorities and the importance-sampling
// weights of the draws (ReplayRing.sample_weights).
#include "bridges_device.h"

namespace bridges {

// Rows of a chunk: the unit of the two-level search.  One workgroup of k_priority_mass covers a chunk, one wave of
// k_priority_draw scans one (four consecutive masses per lane).
constexpr int PRIO_CHUNK = 256;
constexpr double PRIO_CEIL = 1e30;       // a priority above it counts as this much: the total of 2^30 rows stays finite
constexpr double PRIO_FLOOR = 1e-5;      // PrioritizedReplayBuffer's additive floor (replay_memory.py:70-86)

// The mass of one priority.  fmax / fmin return the operand that is not NaN, so a NaN and a negative priority fall to the
// floor and +inf to the ceiling: a diverged step cannot poison the total.  mode 0: alpha == 0, 1: alpha == 1, 2: pow.
__device__ __forceinline__ double prio_mass(double td, double alpha, int mode) {
    const double x = fmin(fmax(td, 0.0), PRIO_CEIL) + PRIO_FLOOR;
    return mode == 1 ? x : (mode == 0 ? 1.0 : pow(x, alpha));
}

// Pass 1: one workgroup per chunk.  Thread j reads the priority of row chunk * 256 + j (one 8-byte read per 8 W-byte row: the
// stride is the record layout's), writes its mass to mass[row] (contiguous; rows past n_rec get 0, so the draw reads whole
// chunks) and the workgroup sums its 256 masses: DPP tree per wave, the four wave sums added in wave order by thread 0.  The
// order is fixed, so chunk_sum is the same bits on every call.
__global__ __launch_bounds__(PRIO_CHUNK) void k_priority_mass(int64_t n_rec, int W, int col, const double* __restrict__ rec, double alpha,
                                                              int mode, double* __restrict__ mass, double* __restrict__ chunk_sum) {
    __shared__ double wave_part[PRIO_CHUNK / WAVE];
    const int64_t row = (int64_t)blockIdx.x * PRIO_CHUNK + threadIdx.x;
    const double m = row < n_rec ? prio_mass(rec[row * W + col], alpha, mode) : 0.0;
    mass[row] = m;
    const double s = wave_sum_d(m);
    if ((threadIdx.x & (WAVE - 1)) == 0) wave_part[threadIdx.x / WAVE] = s;
    __syncthreads();
    if (threadIdx.x == 0) chunk_sum[blockIdx.x] = ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
}

// Pass 2: the inclusive prefix sums of the chunk sums, one workgroup.  Thread t owns the `per` consecutive chunks from t * per:
// it sums them serially, takes as its offset the serial sum of the totals of the threads before it (off_{t+1} = off_t +
// total_t, so the last prefix of thread t IS the offset of thread t + 1) and writes off + the running sum.  chunk_cdf is
// non-decreasing, which the binary search of the draw relies on, and its last entry is the total.
__global__ __launch_bounds__(256) void k_priority_scan(int n_chunks, const double* __restrict__ chunk_sum, double* __restrict__ chunk_cdf) {
    __shared__ double total[256];
    const int per = (n_chunks + 255) / 256;
    const int lo = threadIdx.x * per, hi = min(lo + per, n_chunks);
    double run = 0.0;
    for (int c = lo; c < hi; ++c) run += chunk_sum[c];
    total[threadIdx.x] = run;
    __syncthreads();
    double off = 0.0;
    for (int t = 0; t < (int)threadIdx.x; ++t) off += total[t];
    run = 0.0;
    for (int c = lo; c < hi; ++c) {
        run += chunk_sum[c];
        chunk_cdf[c] = off + run;
    }
}

// Pass 3: one wave per draw, four draws per workgroup.  target = u * total; the chunk is the first whose chunk_cdf exceeds the
// target (binary search, wave-uniform; none: the last chunk), the row the first of the chunk whose prefix
// chunk_cdf[chunk - 1] + (m_0 + .. + m_j) exceeds it (none -- the in-chunk sum is added in another order than the chunk sum and
// may end an ulp short of it: the chunk's last row).  Lane l holds masses 4 l .. 4 l + 3, the lane totals are scanned with six
// shuffle steps.  The result is clamped to n_rec - 1: searchsorted(right=True).clamp(max = n_rec - 1) of the torch path.
__global__ __launch_bounds__(256) void k_priority_draw(int64_t n_rec, int n_chunks, const double* __restrict__ mass,
                                                       const double* __restrict__ chunk_cdf, int64_t n_draws, const double* __restrict__ u,
                                                       int64_t* __restrict__ idx) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t d = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    if (d >= n_draws) return;
    const double target = u[d] * chunk_cdf[n_chunks - 1];
    int lo = 0, hi = n_chunks - 1;                       // the answer lies in [lo, hi]; hi stays the last chunk when none exceeds
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (chunk_cdf[mid] > target) hi = mid; else lo = mid + 1;
    }
    const int c = lo;
    const double base = c > 0 ? chunk_cdf[c - 1] : 0.0;
    const double* m = mass + (int64_t)c * PRIO_CHUNK + 4 * lane;
    const double p0 = m[0], p1 = p0 + m[1], p2 = p1 + m[2], p3 = p2 + m[3];
    double incl = p3;                                    // inclusive scan of the lane totals
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) {
        const double up = __shfl_up(incl, s, WAVE);
        if (lane >= s) incl += up;
    }
    const double before = __shfl_up(incl, 1, WAVE);      // the masses of the lanes below this one
    const double off = lane == 0 ? base : base + before;
    int j = PRIO_CHUNK - 1;
    if (off + p3 > target) j = 4 * lane + 3;
    if (off + p2 > target) j = 4 * lane + 2;
    if (off + p1 > target) j = 4 * lane + 1;
    if (off + p0 > target) j = 4 * lane;
    j = wave_min_i(j);
    int64_t row = (int64_t)c * PRIO_CHUNK + j;
    if (row > n_rec - 1) row = n_rec - 1;
    if (lane == 0) idx[d] = row;
}

// The refresh: rec[idx[j], col] = |q_sa[j] - q_target[j]| as float64.  A row drawn several times takes the value of its LAST
// draw: thread j writes only if no later draw names the same row, which it finds by scanning the later draws, staged through
// LDS a tile of 256 at a time (n is n_steps * batch_size, hundreds: n^2 / 2 compares of LDS words).  Every row is then written
// by exactly one thread -- no race, the same bits on every run.  An index outside [0, n_rec) writes nothing.
__global__ __launch_bounds__(256) void k_priority_update(int64_t n_rec, int W, int col, double* __restrict__ rec, int64_t n,
                                                         const int64_t* __restrict__ idx, const float* __restrict__ q_sa,
                                                         const float* __restrict__ q_target) {
    __shared__ int64_t tile[256];
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t mine = j < n ? idx[j] : -1;
    bool last = j < n && mine >= 0 && mine < n_rec;
    for (int64_t t0 = (int64_t)blockIdx.x * 256; t0 < n; t0 += 256) {     // workgroup-uniform trip count
        const int64_t k = t0 + threadIdx.x;
        tile[threadIdx.x] = k < n ? idx[k] : -1;
        __syncthreads();
        const int cnt = (int)min((int64_t)256, n - t0);
        for (int i = 0; i < cnt; ++i)
            if (t0 + i > j && tile[i] == mine) last = false;
        __syncthreads();
    }
    if (last) rec[mine * W + col] = (double)fabsf(q_sa[j] - q_target[j]);
}

// The importance-sampling weights of the draws (ReplayRing.sample_weights): w_j = (n_rec * m_idx[j] / total)^(-beta), every batch
// of `batch` consecutive draws divided by its own maximum -- n_rec and total cancel: w_j = pow(min_k m_idx[k] / m_idx[j], beta), k
// over the batch of j.  `mass` is what k_priority_mass left in the sampler's scratch: the distribution the draws were made from,
// whatever k_priority_update has written to the record column since.  One workgroup per batch, thread t takes draws t, t + 256, ..;
// the minimum is a DPP tree per wave and the four wave results through LDS (a minimum has no order: the same bits on every call,
// no atomics).  float64 throughout, one rounding to float32.  mode 0: beta == 0 (all ones), 1: beta == 1 (the quotient), 2: pow --
// prio_mass's switch.  An index outside [0, n_rec) takes weight 0 and no part in the minimum (k_priority_update's stance).
__global__ __launch_bounds__(256) void k_priority_weights(int64_t n_rec, int batch, const int64_t* __restrict__ idx,
                                                          const double* __restrict__ mass, double beta, int mode,
                                                          float* __restrict__ weight) {
    __shared__ double wave_part[256 / WAVE];
    const int64_t base = (int64_t)blockIdx.x * batch;
    double lo = INFINITY;                                // masses are finite and positive: never NaN
    for (int k = threadIdx.x; k < batch; k += 256) {
        const int64_t i = idx[base + k];
        if (i >= 0 && i < n_rec) lo = fmin(lo, mass[i]);
    }
    lo = wave_min_d(lo);                                 // every thread is back here: all 64 lanes of the wave take part
    if ((threadIdx.x & (WAVE - 1)) == 0) wave_part[threadIdx.x / WAVE] = lo;
    __syncthreads();
    lo = fmin(fmin(wave_part[0], wave_part[1]), fmin(wave_part[2], wave_part[3]));
    for (int k = threadIdx.x; k < batch; k += 256) {
        const int64_t i = idx[base + k];
        float w = 0.f;
        if (i >= 0 && i < n_rec) {
            const double r = lo / mass[i];               // in (0, 1]; exactly 1 for the row(s) that hold the minimum
            w = mode == 0 ? 1.f : (float)(mode == 1 ? r : pow(r, beta));
        }
        weight[base + k] = w;
    }
}

}  // namespace bridges
