// K7: fused DQN target / soft-update ops (robotoddler/training/successor_dqn.py).
#include "bridges_device.h"

namespace bridges {

// update_target_net (successor_dqn.py:280-288): target = policy * tau + target * (1 - tau), f32, 16 B per lane.
// The two products are rounded separately, as torch does (no FMA: -ffp-contract=off).
__global__ __launch_bounds__(256) void k_soft_update(float* __restrict__ target, const float* __restrict__ policy,
                                                     int64_t n, float tau, float omt) {
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float4* t4 = reinterpret_cast<float4*>(target);
    const float4* p4 = reinterpret_cast<const float4*>(policy);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 t = t4[i], p = p4[i];
        t.x = p.x * tau + t.x * omt;
        t.y = p.y * tau + t.y * omt;
        t.z = p.z * tau + t.z * omt;
        t.w = p.w * tau + t.w * omt;
        t4[i] = t;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        target[i] = policy[i] * tau + target[i] * omt;
}

// One Adam step (struct Adam, bridges_device.h; the optimiser of successor_dqn.py:640) over ONE flat float32 buffer of
// parameters / gradients / moments, 16 B per lane.  t = *step, a device float the caller has ALREADY incremented for this step
// (the fused SuccessorMLP step does it in its loss kernel).
// 7 x 4 B of traffic per parameter (torch's multi-tensor launch moves the same bytes at ~3.9 TB/s: 46 us for the 6.4 M
// parameters of SuccessorMLP; this launch streams them in one grid).
__global__ __launch_bounds__(256) void k_adam_flat(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, const float* __restrict__ step, double lr,
                                                   double beta1_d, double beta2_d, double eps_d) {
    const Adam adam(lr, beta1_d, beta2_d, eps_d, (double)*step);
    const int64_t n4 = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float4* p4 = reinterpret_cast<float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* m4 = reinterpret_cast<float4*>(m);
    float4* v4 = reinterpret_cast<float4*>(v);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 pp = p4[i], gg = g4[i], mm = m4[i], vv = v4[i];
        adam.apply(pp, gg, mm, vv);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float pp = p[i], gg = g[i], mm = m[i], vv = v[i];
        adam.apply(pp, gg, mm, vv);
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
}

// The same update over MANY tensors in one launch (the conv Q-networks: 34-60 parameter tensors of 16 .. 295 k elements, each
// with its own gradient tensor from autograd).  One workgroup per 1024-element chunk of a tensor (chunk_slot / chunk_off name
// the tensor and the chunk's first element): 426 k parameters are ~450 workgroups.  torch's fused multi-tensor launch cuts
// tensors into 64 k-element chunks -- ~40 workgroups for ConvNet, 40 us per step where the bytes are worth 2.
// *step = number of updates done so far (this one is *step + 1; nothing in the launch writes *step, the caller advances it);
// the first chunk of a tensor also writes the new count into the tensor's own step word (torch.optim.Adam's state['step']).
__global__ __launch_bounds__(256) void k_adam_multi(const bridges_adam_slot* __restrict__ slots, const int32_t* __restrict__ chunk_slot,
                                                    const int32_t* __restrict__ chunk_off, const float* __restrict__ step, double lr,
                                                    double beta1_d, double beta2_d, double eps_d) {
    const bridges_adam_slot s = slots[chunk_slot[blockIdx.x]];
    const int64_t base = (int64_t)chunk_off[blockIdx.x] * 1024;
    const double t = (double)*step + 1.0;
    const Adam adam(lr, beta1_d, beta2_d, eps_d, t);
    if (base == 0 && threadIdx.x == 0 && s.step) *s.step = (float)t;
    const int64_t i = base + 4 * (int64_t)threadIdx.x;
    const bool vec = ((((uintptr_t)s.p) | ((uintptr_t)s.g) | ((uintptr_t)s.m) | ((uintptr_t)s.v)) & 15) == 0;
    if (vec && i + 3 < s.n) {
        float4 pp = *reinterpret_cast<float4*>(s.p + i), gg = *reinterpret_cast<const float4*>(s.g + i);
        float4 mm = *reinterpret_cast<float4*>(s.m + i), vv = *reinterpret_cast<float4*>(s.v + i);
        adam.apply(pp, gg, mm, vv);
        *reinterpret_cast<float4*>(s.p + i) = pp; *reinterpret_cast<float4*>(s.m + i) = mm; *reinterpret_cast<float4*>(s.v + i) = vv;
    } else {
        for (int64_t j = i; j < i + 4 && j < s.n; ++j) {
            float pp = s.p[j], gg = s.g[j], mm = s.m[j], vv = s.v[j];
            adam.apply(pp, gg, mm, vv);
            s.p[j] = pp; s.m[j] = mm; s.v[j] = vv;
        }
    }
}

// (value, row) pairs of the segmented arg-max: b replaces a when b holds a row and a holds none, or b's value is greater, or the
// values are equal and b's row is lower.  "Greater value, then lower row" is a TOTAL order on pairs with distinct rows (a pair
// without a row is below all of them), so the maximum of a set of pairs does not depend on the order in which they are combined.
__device__ __forceinline__ void td_take_better(float& av, int& ak, float bv, int bk) {
    if (bk != 0x7fffffff && (ak == 0x7fffffff || bv > av || (bv == av && bk < ak))) { av = bv; ak = bk; }
}

// train_policy_net target construction (successor_dqn.py:197-213, 222, 230), one workgroup per transition: the row is SELECTED
// by one value vector and VALUED by another (double Q-learning; the plain target passes next_q for both),
//   row = first maximum of select_q over [seg_lo[i], seg_hi[i])  (ties to the lowest row; all -inf: the first row),
//   q_target[i] = lin_reward[i] + d_i * (done ? 0 : next_q[row]),  sf_target[i,:] = action_raster[i,:] + d_i * next_sf[row,:],
// d_i = discount[i] (PER_ROW; n-step returns: gamma^h of transition i's horizon) or the scalar gamma.  An empty segment has no
// row (argmax_row 0x7fffffff, q' = -inf, psi' = 0) and a done transition takes q' = 0, psi' = 0.  Every entry point that forms
// a target launches this kernel, so select_q == next_q and a discount filled with gamma give the same bits by construction.
// Reduction for wave64: every thread strides the segment, a wave reduces its 64 pairs by __shfl_down (offsets 32 .. 1; a lane
// whose partner lies beyond the wave gets its own pair back, which changes nothing), the four wave results pass through LDS
// behind ONE barrier and every thread combines the four.  Because the order of pairs is total (td_take_better) the result does
// not depend on the shape of the reduction.
// The successor-feature row goes 16 B per lane when sf_dim and the row stride are multiples of 4 floats and the three bases are
// 16-byte aligned, element by element otherwise (sf_dim = 6): the same float operations per element either way.
template <bool PER_ROW>
__global__ __launch_bounds__(256) void k_td_target(int n_trans, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                   const float* __restrict__ select_q, const float* __restrict__ next_q,
                                                   const float* __restrict__ next_sf, int64_t sf_row_stride,
                                                   const float* __restrict__ action_raster, const float* __restrict__ lin_reward,
                                                   const uint8_t* __restrict__ done, const float* __restrict__ discount,
                                                   float gamma_scalar, int sf_dim, float* __restrict__ q_target,
                                                   float* __restrict__ sf_target, int32_t* __restrict__ argmax_row) {
    __shared__ float s_val[4];
    __shared__ int s_idx[4];
    const int i = blockIdx.x, t = threadIdx.x;
    if (i >= n_trans) return;                            // (uniform per workgroup: the grid is n_trans)
    const int lo = seg_lo[i], hi = seg_hi[i];
    float gamma = gamma_scalar;
    if constexpr (PER_ROW) gamma = discount[i];
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int j = lo + t; j < hi; j += 256) {
        float v = select_q[j];
        if (v > best || (v == best && j < bidx) || bidx == 0x7fffffff) { best = v; bidx = j; }   // NaN-free inputs
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const float v = __shfl_down(best, o, WAVE);
        const int k = __shfl_down(bidx, o, WAVE);
        td_take_better(best, bidx, v, k);
    }
    if ((t & (WAVE - 1)) == 0) { s_val[t / WAVE] = best; s_idx[t / WAVE] = bidx; }
    __syncthreads();
    best = s_val[0]; bidx = s_idx[0];
#pragma unroll
    for (int w = 1; w < 256 / WAVE; ++w) td_take_better(best, bidx, s_val[w], s_idx[w]);
    const int row = bidx;
    const bool dn = done[i] != 0;
    const bool no_next = dn || row == 0x7fffffff;       // an empty segment has no next row: nothing of next_q / next_sf is read for it
    if (t == 0) {
        float nq = dn ? 0.f : (row == 0x7fffffff ? -INFINITY : next_q[row]);
        q_target[i] = lin_reward[i] + gamma * nq;
        argmax_row[i] = row;
    }
    if (sf_dim > 0) {
        const float* src = next_sf + (int64_t)(no_next ? 0 : row) * sf_row_stride;
        const float* ar = action_raster + (int64_t)i * sf_dim;
        float* dst = sf_target + (int64_t)i * sf_dim;
        const bool vec = (((int64_t)sf_dim | sf_row_stride) & 3) == 0 &&
                         ((((uintptr_t)next_sf) | ((uintptr_t)action_raster) | ((uintptr_t)sf_target)) & 15) == 0;
        const int n4 = vec ? sf_dim >> 2 : 0;
        for (int k = t; k < n4; k += 256) {
            float4 a = reinterpret_cast<const float4*>(ar)[k];
            float4 s = no_next ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<const float4*>(src)[k];
            float4 o;
            o.x = a.x + gamma * s.x; o.y = a.y + gamma * s.y; o.z = a.z + gamma * s.z; o.w = a.w + gamma * s.w;
            reinterpret_cast<float4*>(dst)[k] = o;
        }
        for (int k = (n4 << 2) + t; k < sf_dim; k += 256) dst[k] = ar[k] + gamma * (no_next ? 0.f : src[k]);
    }
}

// The n-step fold of one lock-step's one-step records (robotoddler/training/vec_dqn.py, DESIGN.md "n-step returns"): every env
// keeps a window of up to n pending starts -- the return accumulated so far, the discount of the next reward, and the start's
// stable(s) flag and priority -- and per valid transition
//   1. a start is appended (acc 0, disc 1, the record's STABLE_S and TD),
//   2. every pending start j takes the reward: acc_j += disc_j * lin, disc_j *= gamma            (float64),
//   3. a done record emits every pending start, oldest first, with horizon h_j = count - j, and empties the window; otherwise a
//      full window (count == n) emits its oldest start with h = n and shifts the rest down.
// An emitted row is the CURRENT record (block list, action, DONE, STABLE_N, REWARD, task tail: the last step's) with LIN = acc_j,
// STABLE_S and TD = the start's, and h_j in the new last column W.  Env e's rows are out[e * n ...], oldest first; out_valid marks
// them, the rest of the env's n rows is not written.  An env without a valid transition keeps its window and emits nothing.
// One wave per env, four envs per workgroup: the window update is wave-uniform (every lane holds the window in registers, lane 0
// writes it back), the lanes stride the columns of the row copies (8-byte accesses, consecutive lanes on consecutive doubles).
// No atomics, no count: the caller sums out_valid.
__global__ __launch_bounds__(256) void k_nstep_fold(int E, int W, int n, const double* __restrict__ rec, const uint8_t* __restrict__ valid,
                                                    double gamma, int32_t* __restrict__ count, double* __restrict__ acc,
                                                    double* __restrict__ disc, double* __restrict__ stable_s, double* __restrict__ td,
                                                    double* __restrict__ out, uint8_t* __restrict__ out_valid) {
    constexpr int N = BRIDGES_NSTEP_MAX;
    const int lane = threadIdx.x & (WAVE - 1);
    const int e = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    if (e >= E) return;
    const double* row = rec + (size_t)e * W;
    int n_emit = 0, c = 0;
    double a[N], d[N], ss[N], pr[N];
    if (valid[e]) {
        c = count[e];
        c = c < 0 ? 0 : (c > n - 1 ? n - 1 : c);            // the invariant of the window: at most n - 1 starts are pending here
        const double lin = row[BRIDGES_REC_LIN], r_ss = row[BRIDGES_REC_STABLE_S], r_td = row[BRIDGES_REC_TD];
        const bool dn = row[BRIDGES_REC_DONE] > 0.5;
        const size_t w0 = (size_t)e * n;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const bool live = j < c;
            a[j] = live ? acc[w0 + j] : 0.0;
            d[j] = live ? disc[w0 + j] : 1.0;
            ss[j] = live ? stable_s[w0 + j] : r_ss;         // slot c is the appended start; the slots above it are never read
            pr[j] = live ? td[w0 + j] : r_td;
        }
        c += 1;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            if (j < c) {
                a[j] += d[j] * lin;
                d[j] *= gamma;
            }
        }
        n_emit = dn ? c : (c == n ? 1 : 0);
        // the window after the emissions: empty, shifted down by one, or as it is
        const int keep = dn ? 0 : c - n_emit;
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                if (j < keep) {
                    const int s = (j + 1 < N) ? j + 1 : j;
                    acc[w0 + j] = n_emit ? a[s] : a[j];
                    disc[w0 + j] = n_emit ? d[s] : d[j];
                    stable_s[w0 + j] = n_emit ? ss[s] : ss[j];
                    td[w0 + j] = n_emit ? pr[s] : pr[j];
                }
            }
            count[e] = keep;
        }
    }
    if (lane < n) out_valid[(size_t)e * n + lane] = lane < n_emit;
    if (n_emit == 0) return;
    const int Wo = W + 1;
    double* dst = out + (size_t)e * n * Wo;
    for (int c0 = 0; c0 < Wo; c0 += WAVE) {
        const int col = c0 + lane;
        const double v = col < W ? row[col] : 0.0;
#pragma unroll
        for (int r = 0; r < N; ++r) {
            if (r < n_emit && col < Wo) {
                double o = v;
                if (col == BRIDGES_REC_LIN) o = a[r];
                if (col == BRIDGES_REC_STABLE_S) o = ss[r];
                if (col == BRIDGES_REC_TD) o = pr[r];
                if (col == W) o = (double)(c - r);
                dst[(size_t)r * Wo + col] = o;
            }
        }
    }
}

// acc += the rows of wt at the set pixels of one bit-packed raster, ascending p (lane l holds image row l in `mine`, rows_nz is
// the ballot of the non-empty rows): the walk of both first-layer kernels below.
__device__ __forceinline__ void bits_linear_add(float4& acc, uint64_t mine, uint64_t rows_nz, const float* __restrict__ wt, int d,
                                                int col, bool act) {
    uint64_t rem = rows_nz;
    while (rem) {
        const int rr = __builtin_ctzll(rem);
        rem &= rem - 1ull;
        uint64_t m = shfl_u64(mine, rr);                                     // uniform: the mask of image row rr
        const float* w = wt + (size_t)rr * IMG * d + col;
        while (m) {
            const int cc = __builtin_ctzll(m);
            m &= m - 1ull;
            if (act) {
                const float4 v = *reinterpret_cast<const float4*>(w + (size_t)cc * d);
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
        }
    }
}

// K8: first layer of an MLP that consumes flattened binary 64x64 rasters, fed with the bit-packed rasters themselves
// (cv.py:95-97 concatenates block / action / reward / obstacle images and multiplies by W1; a block covers ~35 of the
// 4096 pixels, so the product with its raster is the sum of ~35 rows of the transposed weight slice):
//   out[r, :] = base[base_row[r], :] + sum over set pixels p of bits[bits_row[r]] (ascending p) of wt[p, :]
// One wave per output row, 16 B per lane; wt (4 MiB for d = 256) stays in L2.
__global__ __launch_bounds__(256) void k_bits_linear(int n_rows, const uint64_t* __restrict__ bits,
                                                     const int64_t* __restrict__ bits_row, const float* __restrict__ wt,
                                                     int d, const float* __restrict__ base,
                                                     const int64_t* __restrict__ base_row, float* __restrict__ out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int nwaves = (gridDim.x * blockDim.x) / WAVE;
    for (int rv = wave; rv < n_rows; rv += nwaves) {
        const int r = __builtin_amdgcn_readfirstlane(rv);
        const int64_t src = bits_row ? bits_row[r] : (int64_t)r;
        const uint64_t mine = bits[(size_t)src * IMG + lane];               // image row `lane`
        const uint64_t rows_nz = __ballot(mine != 0ull);
        const float* b = base ? base + (size_t)(base_row ? base_row[r] : 0) * d : nullptr;
        for (int c0 = 0; c0 < d; c0 += 4 * WAVE) {
            const int col = c0 + 4 * lane;
            const bool act = col < d;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (b && act) acc = *reinterpret_cast<const float4*>(b + col);
            bits_linear_add(acc, mine, rows_nz, wt, d, col, act);
            if (act) *reinterpret_cast<float4*>(out + (size_t)r * d + col) = acc;
        }
    }
}

// K8 with two bit-packed operands (per-env obstacles: state raster x W_block + the env's obstacle raster x W_obst):
//   out[r, :] = base[base_row[r], :] + sum over set pixels p of bits_a[row_a[r]] of wt_a[p, :]
//                                     + sum over set pixels p of bits_b[row_b[r]] of wt_b[p, :]
// summed in exactly that order, pixels ascending inside an operand: the float sequence of two chained k_bits_linear launches
// (the second with the first's output as its base, row r), so the result equals theirs bit for bit -- without the store and
// reload of the intermediate row and the second launch.  Both row masks stay in the wave (one uint64 per lane each).
__global__ __launch_bounds__(256) void k_bits_linear2(int n_rows, const uint64_t* __restrict__ bits_a,
                                                      const int64_t* __restrict__ row_a, const float* __restrict__ wt_a,
                                                      const uint64_t* __restrict__ bits_b, const int64_t* __restrict__ row_b,
                                                      const float* __restrict__ wt_b, int d, const float* __restrict__ base,
                                                      const int64_t* __restrict__ base_row, float* __restrict__ out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int nwaves = (gridDim.x * blockDim.x) / WAVE;
    for (int rv = wave; rv < n_rows; rv += nwaves) {
        const int r = __builtin_amdgcn_readfirstlane(rv);
        const int64_t src_a = row_a ? row_a[r] : (int64_t)r;
        const int64_t src_b = row_b ? row_b[r] : (int64_t)r;
        const uint64_t mine_a = bits_a[(size_t)src_a * IMG + lane];         // image row `lane` of either operand
        const uint64_t mine_b = bits_b[(size_t)src_b * IMG + lane];
        const uint64_t nz_a = __ballot(mine_a != 0ull);
        const uint64_t nz_b = __ballot(mine_b != 0ull);
        const float* b = base ? base + (size_t)(base_row ? base_row[r] : 0) * d : nullptr;
        for (int c0 = 0; c0 < d; c0 += 4 * WAVE) {
            const int col = c0 + 4 * lane;
            const bool act = col < d;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (b && act) acc = *reinterpret_cast<const float4*>(b + col);
            bits_linear_add(acc, mine_a, nz_a, wt_a, d, col, act);
            bits_linear_add(acc, mine_b, nz_b, wt_b, d, col, act);
            if (act) *reinterpret_cast<float4*>(out + (size_t)r * d + col) = acc;
        }
    }
}

// Count-based exploration of EpsilonGreedy (successor_dqn.py:112-131) on the bit-packed rasters, both directions:
//   k_bits_dot:        out[r] = sum over the set pixels of bits[bits_row[r]] of img[slot[r]]  (= sum(step_images[step] * a_r))
//   k_bits_accumulate: img[slot[r]] += weight[r] * raster(bits[bits_row[r]])                  (= step_images[step] += a_sel)
// One wave per row, lane = image row: a raster holds ~35 pixels, so a lane walks the handful of set bits of its own row
// instead of a [n, 4096] product / a [n, 64, 64] float image.  The images hold small integer counts: float sums of them
// are exact in any order, so neither the wave reduction nor the float atomics change a bit of the result.
__global__ __launch_bounds__(256) void k_bits_dot(int n_rows, const uint64_t* __restrict__ bits, const int64_t* __restrict__ bits_row,
                                                  const float* __restrict__ img, const int64_t* __restrict__ slot,
                                                  float* __restrict__ out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int nwaves = (gridDim.x * blockDim.x) / WAVE;
    for (int rv = wave; rv < n_rows; rv += nwaves) {
        const int r = __builtin_amdgcn_readfirstlane(rv);
        const int64_t src = bits_row ? bits_row[r] : (int64_t)r;
        uint64_t m = bits[(size_t)src * IMG + lane];
        const float* row = img + ((size_t)slot[r] * IMG + lane) * IMG;
        double acc = 0.0;
        while (m) {
            const int x = __builtin_ctzll(m);
            m &= m - 1ull;
            acc += (double)row[x];
        }
        acc = wave_sum_d(acc);
        if (lane == 0) out[r] = (float)acc;
    }
}

__global__ __launch_bounds__(256) void k_bits_accumulate(int n_rows, const uint64_t* __restrict__ bits,
                                                         const int64_t* __restrict__ bits_row, const float* __restrict__ weight,
                                                         const int64_t* __restrict__ slot, float* __restrict__ img) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int nwaves = (gridDim.x * blockDim.x) / WAVE;
    for (int rv = wave; rv < n_rows; rv += nwaves) {
        const int r = __builtin_amdgcn_readfirstlane(rv);
        const float w = weight ? weight[r] : 1.f;
        if (w == 0.f) continue;
        const int64_t src = bits_row ? bits_row[r] : (int64_t)r;
        uint64_t m = bits[(size_t)src * IMG + lane];
        float* row = img + ((size_t)slot[r] * IMG + lane) * IMG;
        while (m) {
            const int x = __builtin_ctzll(m);
            m &= m - 1ull;
            atomicAdd(row + x, w);
        }
    }
}

// Head of the factored acting forward: q[r] = sum_j w[j] * sigmoid(d[r, j])  (cv.py:101-104: softmax over the two successor
// channels, channel 1, times the reward map, summed over the image) in ONE pass over d instead of sigmoid / mul / sum
// passes.  One wave per row, 16 B per lane per trip; lane partial sums in f32, the 64 partials added in f64.
// PER_ROW (per-env tasks): w is [M, k] and row r is weighed with map w_row[r].
template <bool PER_ROW>
__global__ __launch_bounds__(256) void k_sigmoid_dot(int n_rows, const float* __restrict__ d, int64_t row_stride,
                                                     const float* __restrict__ w_all, const int32_t* __restrict__ w_row, int k,
                                                     float* __restrict__ out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int nwaves = (gridDim.x * blockDim.x) / WAVE;
    for (int r = wave; r < n_rows; r += nwaves) {
        const float* row = d + (size_t)r * row_stride;
        const float* w = PER_ROW ? w_all + (size_t)w_row[r] * k : w_all;
        float acc = 0.f;
        // four 16-B loads of the row in flight per lane and trip (a 64 x 64 image: four trips), the sigmoid through the
        // hardware reciprocal (1 ulp; a full float32 division is ~10 instructions per pixel and made the pass ALU-heavy)
#define SIGDOT_ONE(X, WW)                                                     \
    acc += WW.x * __builtin_amdgcn_rcpf(1.f + __expf(-X.x));                 \
    acc += WW.y * __builtin_amdgcn_rcpf(1.f + __expf(-X.y));                 \
    acc += WW.z * __builtin_amdgcn_rcpf(1.f + __expf(-X.z));                 \
    acc += WW.w * __builtin_amdgcn_rcpf(1.f + __expf(-X.w));
        int j = 4 * lane;
        for (; j + 12 * WAVE < k; j += 16 * WAVE) {
            const float4 x0 = *reinterpret_cast<const float4*>(row + j), x1 = *reinterpret_cast<const float4*>(row + j + 4 * WAVE);
            const float4 x2 = *reinterpret_cast<const float4*>(row + j + 8 * WAVE), x3 = *reinterpret_cast<const float4*>(row + j + 12 * WAVE);
            const float4 w0 = *reinterpret_cast<const float4*>(w + j), w1 = *reinterpret_cast<const float4*>(w + j + 4 * WAVE);
            const float4 w2 = *reinterpret_cast<const float4*>(w + j + 8 * WAVE), w3 = *reinterpret_cast<const float4*>(w + j + 12 * WAVE);
            SIGDOT_ONE(x0, w0) SIGDOT_ONE(x1, w1) SIGDOT_ONE(x2, w2) SIGDOT_ONE(x3, w3)
        }
        for (; j < k; j += 4 * WAVE) {
            const float4 x = *reinterpret_cast<const float4*>(row + j);
            const float4 ww = *reinterpret_cast<const float4*>(w + j);
            SIGDOT_ONE(x, ww)
        }
#undef SIGDOT_ONE
        const double total = wave_sum_d((double)acc);
        if (lane == 0) out[r] = (float)total;
    }
}

// ---- inference epilogues of the conv nets (robotoddler/models/cv.py: Conv2d -> ReLU [-> MaxPool2d(2)]) -------------
// torch runs "+ bias", "relu" and "maxpool" as three passes over the activation tensor (9.3 GB of traffic per 2048
// rows of the ConvNet, a third of its forward time); these do them in one.  Adding the channel's bias and clamping at
// zero are monotone, so max(x_i) + b -> relu gives bit for bit what pool(relu(x_i + b)) gives.
// x [n, C, hw] contiguous (NCHW), hw % 4 == 0; in place.
__global__ __launch_bounds__(256) void k_bias_relu(float* __restrict__ x, const float* __restrict__ bias, int64_t n4,
                                                   int hw4, int C) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    float4* x4 = reinterpret_cast<float4*>(x);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float b = bias[(i / hw4) % C];
        float4 v = x4[i];
        v.x = relu_nan(v.x + b); v.y = relu_nan(v.y + b); v.z = relu_nan(v.z + b); v.w = relu_nan(v.w + b);
        x4[i] = v;
    }
}

// out[nc, H/2, W/2] = relu(max over the 2x2 window of x[nc, H, W] + bias[c]); W % 4 == 0, H % 2 == 0.
// One thread: 4 input columns of 2 rows -> 2 outputs.
__global__ __launch_bounds__(256) void k_bias_relu_pool2(const float* __restrict__ x, const float* __restrict__ bias,
                                                         float* __restrict__ out, int64_t n_items, int H, int W, int C) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int w4 = W >> 2, h2 = H >> 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_items; i += stride) {
        const int64_t q = i % w4, rest = i / w4;
        const int64_t r = rest % h2, nc = rest / h2;
        const float b = bias[nc % C];
        const float* p = x + (nc * H + 2 * r) * W + 4 * q;
        const float4 a0 = *reinterpret_cast<const float4*>(p), a1 = *reinterpret_cast<const float4*>(p + W);
        float2 o;
        o.x = relu_nan(max4_nan(a0.x, a0.y, a1.x, a1.y) + b);
        o.y = relu_nan(max4_nan(a0.z, a0.w, a1.z, a1.w) + b);
        *reinterpret_cast<float2*>(out + (nc * h2 + r) * (W >> 1) + 2 * q) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// EpsilonGreedy.select (successor_dqn.py:98-132) for every env of the vectorised loop in one launch: per env, over its rows
// seg[e] .. seg[e + 1] of the Q pass, the greedy row = first maximum of q, the exploring row = first minimum of the overlap
// `join` of the candidate with the count image of the env's episode step (count-based exploration); the env explores when
// its uniform draw u[e] <= eps (and the call is not greedy).  An env without rows gets row 0 with weight 0.  The rows of
// env e are seg_lo[e] .. seg_hi[e] (envs in the same state share their representative's rows, rep[e]: the compact index of
// the chosen row is then a candidate of the REPRESENTATIVE, whose candidates are env e's own, one for one).  Replaces two
// segmented arg-max launches and ~20 element-wise / index launches.  One wave per env.
//   sel_compact[e] = idx[row]  (compact candidate index), sel_index[e] = sel_compact - cand_offset[rep[e]] (>= 0),
//   q_sel[e] = q[row] (0 without rows), explore_w[e] = 1.0 if the env explored and has rows else 0.0
__global__ __launch_bounds__(256) void k_eps_greedy_select(int E, int n_rows, const int32_t* __restrict__ seg_lo,
                                                           const int32_t* __restrict__ seg_hi, const float* __restrict__ q,
                                                           const float* __restrict__ join, const float* __restrict__ u, float eps,
                                                           int greedy, const int64_t* __restrict__ idx,
                                                           const int32_t* __restrict__ cand_offset, const int32_t* __restrict__ rep,
                                                           int64_t* __restrict__ sel_compact,
                                                           int32_t* __restrict__ sel_index, float* __restrict__ q_sel,
                                                           float* __restrict__ explore_w) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= E) return;
    const int lo = seg_lo[e], hi = seg_hi[e];
    const bool explore = !greedy && u[e] <= eps;
    // first maximum of q, or of -join (= first minimum of join), over the env's rows
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int j = lo + lane; j < hi; j += 64) {
        const float v = explore ? -join[j] : q[j];
        if (bi == 0x7fffffff || v > best || (v == best && j < bi)) { best = v; bi = j; }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const float v = __shfl_xor(best, m);
        const int k = __shfl_xor(bi, m);
        if (k != 0x7fffffff && (bi == 0x7fffffff || v > best || (v == best && k < bi))) { best = v; bi = k; }
    }
    if (lane == 0) {
        const bool has = hi > lo;
        int row = has ? bi : 0;
        if (row > n_rows - 1) row = n_rows - 1;
        const int64_t c = idx[row];
        sel_compact[e] = c;
        const int64_t rel = c - (int64_t)cand_offset[rep ? rep[e] : e];
        sel_index[e] = rel > 0 ? (int32_t)rel : 0;
        q_sel[e] = has ? q[row] : 0.f;
        explore_w[e] = (explore && has) ? 1.f : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Boltzmann exploration (the reference's Softmax policy, successor_dqn.py:138-154, made to run) for every env of the vectorised
// loop in one launch: env e draws row j of its rows lo .. hi - 1 of the Q pass with probability proportional to
//   w_j = exp((q_j - m) / T),  m = the largest q of the env that is neither NaN nor -inf (such rows weigh 0; m = +inf: the +inf
//   rows weigh 1, all others 0),
// by the inverse CDF: c_j = w_lo + .. + w_j in row order, the row is the first with c_j > u[e] * total (strict; none, by rounding:
// the last row with w_j > 0).  No eligible row: row lo with p_sel 0.  The rule in full stands in include/bridges_hip.h.
// One wave per env, three passes over its rows: the maximum (lane-strided, DPP tree), the total (64 rows at a time, DPP tree per
// chunk, chunks added in order) and the search (64 rows at a time, shuffle scan as in k_priority_draw, a running carry from chunk
// to chunk; it stops at the first chunk that holds the row).  float64 throughout: (q - m) / T reaches -745 before a weight
// underflows, and a float32 prefix sum over hundreds of rows would move draws near a boundary to the neighbouring row; p_sel is
// rounded to float32 once.  No atomics, no LDS, a fixed order of additions: the same bits on every call.  lo and hi are made
// scalar, so every lane runs every chunk and reaches every cross-lane step.  greedy != 0: the row of
// k_eps_greedy_select(greedy = 1), by its very loop.
//   sel_compact / sel_index / q_sel as k_eps_greedy_select writes them; explore_w[e] = 1.0 if the env has rows and the drawn row
//   is not the first maximum among its eligible rows, else 0.0; p_sel[e] = w_row / total (greedy: 1; no rows, no eligible row: 0).
__device__ __forceinline__ double boltzmann_weight(float qv, double m, double T) {
    if (!(qv == qv) || qv == -INFINITY) return 0.0;
    if (m == (double)INFINITY) return qv == INFINITY ? 1.0 : 0.0;
    return exp(((double)qv - m) / T);
}

// The spread of a segment (the relative-temperature operators; the rule stands in include/bridges_hip.h): the population standard
// deviation of the rows lo .. hi - 1 of q that are neither NaN nor +-inf, 0 if fewer than two are.  Two passes -- the mean, then the
// squared deviations from it, never E[x^2] - mean^2 --, float64 throughout.  The lane `first` of STRIDE takes the rows lo + first,
// lo + first + STRIDE, ..; `combine` makes the segment's sum of a wave's (wave_sum_d's DPP tree): the identity where one wave owns
// the segment (k_boltzmann_select), the LDS wave-combine of phase A in k_soft_expect, a fresh slot per call.  Every lane that
// `combine` joins must call this, and all of them get the same bits back.
template <int STRIDE, class Combine>
__device__ __forceinline__ double segment_spread(const float* q, int lo, int hi, int first, Combine combine) {
    double sum = 0.0, cnt = 0.0;
    for (int j = lo + first; j < hi; j += STRIDE) {
        const float v = q[j];
        if (isfinite(v)) { sum += (double)v; cnt += 1.0; }
    }
    sum = combine(wave_sum_d(sum), 0);
    const double n_f = combine(wave_sum_d(cnt), 1);      // (a count below 2^53: exact in any order)
    if (n_f < 2.0) return 0.0;                           // uniform over the lanes `combine` joins
    const double mean = sum / n_f;
    double dev = 0.0;
    for (int j = lo + first; j < hi; j += STRIDE) {
        const float v = q[j];
        if (isfinite(v)) { const double d = (double)v - mean; dev += d * d; }
    }
    return sqrt(combine(wave_sum_d(dev), 2) / n_f);
}
// T_e = temperature * max(spread, floor); both factors are > 0 and finite, so is the product unless it overflows a double's range
__device__ __forceinline__ double relative_temperature(float temperature, double spread, float spread_floor) {
    return (double)temperature * fmax(spread, (double)spread_floor);
}

// One body for k_boltzmann_select and k_boltzmann_select_rel.  REL: the temperature of env e is relative_temperature() of the
// spread of its rows, taken between pass 1 and pass 2 and written to temp_out[e] (greedy: 0; no rows or no eligible row: no row
// is finite either, so temperature * spread_floor without a pass).
template <bool REL>
__device__ __forceinline__ void boltzmann_select_body(int E, int n_rows, const int32_t* __restrict__ seg_lo,
                                                      const int32_t* __restrict__ seg_hi, const float* __restrict__ q,
                                                      const float* __restrict__ u, float temperature, float spread_floor, int greedy,
                                                      const int64_t* __restrict__ idx, const int32_t* __restrict__ cand_offset,
                                                      const int32_t* __restrict__ rep, int64_t* __restrict__ sel_compact,
                                                      int32_t* __restrict__ sel_index, float* __restrict__ q_sel,
                                                      float* __restrict__ explore_w, float* __restrict__ p_sel,
                                                      double* __restrict__ temp_out) {
    constexpr int NONE = 0x7fffffff;
    const int lane = threadIdx.x & (WAVE - 1);
    const int e = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    if (e >= E) return;                                  // wave-uniform: e is the same in all 64 lanes
    const int lo = __builtin_amdgcn_readfirstlane(seg_lo[e]), hi = __builtin_amdgcn_readfirstlane(seg_hi[e]);
    const bool has = hi > lo;
    int row = NONE, first_max = NONE;
    double p = 0.0;
    double t_e = REL ? (greedy ? 0.0 : relative_temperature(temperature, 0.0, spread_floor)) : 0.0;
    if (greedy) {
        // k_eps_greedy_select's search, operand for operand (it decides what a NaN row does to the choice)
        float best = -INFINITY;
        int bi = NONE;
        for (int j = lo + lane; j < hi; j += 64) {
            const float v = q[j];
            if (bi == NONE || v > best || (v == best && j < bi)) { best = v; bi = j; }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const float v = __shfl_xor(best, m);
            const int k = __shfl_xor(bi, m);
            if (k != NONE && (bi == NONE || v > best || (v == best && k < bi))) { best = v; bi = k; }
        }
        row = first_max = bi;
        p = has ? 1.0 : 0.0;
    } else if (has) {
        double T = (double)temperature;
        // pass 1: the largest eligible q (-inf: no row is eligible)
        double mx = -INFINITY;
        for (int j = lo + lane; j < hi; j += 64) {
            const float v = q[j];
            if (v == v && (double)v > mx) mx = (double)v;
        }
        const double m = wave_max_d(mx);
        if (m == -(double)INFINITY) {
            row = first_max = lo;
        } else {
            if (REL) {
                T = t_e = relative_temperature(temperature, segment_spread<WAVE>(q, lo, hi, lane, [](double v, int) { return v; }),
                                               spread_floor);
            }
            // pass 2: the total, and the first row that holds the maximum
            double total = 0.0;
            int fm = NONE;
            for (int base = lo; base < hi; base += 64) {
                const int j = base + lane;
                const float v = j < hi ? q[j] : -INFINITY;
                if (fm == NONE && (double)v == m) fm = j;
                total += wave_sum_d(boltzmann_weight(v, m, T));
            }
            first_max = wave_min_i(fm);
            // pass 3: the first row whose prefix exceeds the target
            const double target = (double)u[e] * total;
            double carry = 0.0;
            int last_pos = -1;                            // this lane's last row of positive weight
            int found = NONE;
            for (int base = lo; base < hi; base += 64) {
                const int j = base + lane;
                const double w = boltzmann_weight(j < hi ? q[j] : -INFINITY, m, T);
                double incl = w;                          // inclusive scan of the chunk's weights
#pragma unroll
                for (int s = 1; s < WAVE; s <<= 1) {
                    const double up = __shfl_up(incl, s, WAVE);
                    if (lane >= s) incl += up;
                }
                if (w > 0.0) last_pos = j;
                found = wave_min_i((j < hi && carry + incl > target) ? j : NONE);
                if (found != NONE) break;                 // wave-uniform: wave_min_i returns a scalar
                carry += readlane_d(incl, WAVE - 1);
            }
            if (found == NONE) found = -wave_min_i(-last_pos);        // rounding left none: the last row that weighs anything
            row = found;
            p = boltzmann_weight(q[row], m, T) / total;
        }
    }
    if (lane == 0) {
        const bool explored = has && !greedy && row != first_max;
        if (!has) row = 0;
        if (row > n_rows - 1) row = n_rows - 1;
        const int64_t c = idx[row];
        sel_compact[e] = c;
        const int64_t rel = c - (int64_t)cand_offset[rep ? rep[e] : e];
        sel_index[e] = rel > 0 ? (int32_t)rel : 0;
        q_sel[e] = has ? q[row] : 0.f;
        explore_w[e] = explored ? 1.f : 0.f;
        p_sel[e] = (float)p;
        if (REL) temp_out[e] = t_e;
    }
}

__global__ __launch_bounds__(256) void k_boltzmann_select(int E, int n_rows, const int32_t* __restrict__ seg_lo,
                                                          const int32_t* __restrict__ seg_hi, const float* __restrict__ q,
                                                          const float* __restrict__ u, float temperature, int greedy,
                                                          const int64_t* __restrict__ idx, const int32_t* __restrict__ cand_offset,
                                                          const int32_t* __restrict__ rep, int64_t* __restrict__ sel_compact,
                                                          int32_t* __restrict__ sel_index, float* __restrict__ q_sel,
                                                          float* __restrict__ explore_w, float* __restrict__ p_sel) {
    boltzmann_select_body<false>(E, n_rows, seg_lo, seg_hi, q, u, temperature, 0.f, greedy, idx, cand_offset, rep, sel_compact, sel_index,
                                 q_sel, explore_w, p_sel, nullptr);
}

__global__ __launch_bounds__(256) void k_boltzmann_select_rel(int E, int n_rows, const int32_t* __restrict__ seg_lo,
                                                              const int32_t* __restrict__ seg_hi, const float* __restrict__ q,
                                                              const float* __restrict__ u, float temperature, float spread_floor,
                                                              int greedy, const int64_t* __restrict__ idx,
                                                              const int32_t* __restrict__ cand_offset, const int32_t* __restrict__ rep,
                                                              int64_t* __restrict__ sel_compact, int32_t* __restrict__ sel_index,
                                                              float* __restrict__ q_sel, float* __restrict__ explore_w,
                                                              float* __restrict__ p_sel, double* __restrict__ temp_out) {
    boltzmann_select_body<true>(E, n_rows, seg_lo, seg_hi, q, u, temperature, spread_floor, greedy, idx, cand_offset, rep, sel_compact,
                                sel_index, q_sel, explore_w, p_sel, temp_out);
}

// ---------------------------------------------------------------------------------------------------------------
// Transition records of the vectorised loop (robotoddler/training/records.py: one float64 row per transition, the
// compact form of the reference's Transition, successor_dqn.py:27-44; layout BRIDGES_REC_* of the header).  The torch
// formulation of these three steps was ~95 slice / cast / index launches of a few microseconds per lock-step.
//   k_record_state:   before step(): the state s of every env and the chosen candidate -> rec[:, 0 : REC_REWARD], stable(s)
//   k_record_result:  after step():  reward, lin_reward, done | no_actions, stable(s') -> rec, valid_step -> valid
//   k_replay_unpack:  sampled records -> the replay env's state arrays holding s' = s + the action block with the
//                     occupancy update of gym_env.py:228-232, the candidate count of s', the block ranges of s' and s
// One 64-lane workgroup per env / record, lane k = block slot k.
__global__ __launch_bounds__(64) void k_record_state(int E, int K, const int32_t* __restrict__ n_blocks,
                                                     const int32_t* __restrict__ blk_shape, const double* __restrict__ blk_pose,
                                                     const uint8_t* __restrict__ blk_occ, const uint8_t* __restrict__ step_flags,
                                                     const int64_t* __restrict__ sel_row, const int32_t* __restrict__ cand_desc,
                                                     const double* __restrict__ cand_pose, double* __restrict__ rec) {
    const int e = blockIdx.x, k = threadIdx.x;
    if (e >= E) return;
    double* r = rec + (size_t)e * BRIDGES_REC_WIDTH;
    for (int c = k; c < BRIDGES_REC_WIDTH; c += 64) r[c] = 0.0;        // slots >= K, td_error
    __syncthreads();
    if (k < K) {
        r[BRIDGES_REC_SHAPE + k] = (double)blk_shape[(size_t)e * K + k];
        const double* p = blk_pose + ((size_t)e * K + k) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[BRIDGES_REC_POSE + 4 * k + j] = p[j];
        r[BRIDGES_REC_OCC + k] = (double)blk_occ[(size_t)e * K + k];
    }
    if (k == 0) {
        const int nb = n_blocks[e];
        r[BRIDGES_REC_NB] = (double)nb;
        const int64_t row = sel_row[e];
        const int32_t* d = cand_desc + row * 4;                            // (target_block, target_face, shape, face)
        r[BRIDGES_REC_ASHAPE] = (double)d[2];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[BRIDGES_REC_APOSE + j] = cand_pose[row * 4 + j];
        r[BRIDGES_REC_ATB] = (double)d[0];
        r[BRIDGES_REC_ATF] = (double)d[1];
        r[BRIDGES_REC_AFACE] = (double)d[3];
        // 'stable' of s: a freshly reset env is stable (stability.py:53-56), else the frozen verdict of the last step
        r[BRIDGES_REC_STABLE_S] = (nb == 0 || step_flags[(size_t)e * 8 + 1]) ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(256) void k_record_result(int E, const float* __restrict__ reward, const float* __restrict__ lin_reward,
                                                       const uint8_t* __restrict__ step_flags, double* __restrict__ rec,
                                                       uint8_t* __restrict__ valid) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const uint8_t* f = step_flags + (size_t)e * 8;
    double* r = rec + (size_t)e * BRIDGES_REC_WIDTH;
    r[BRIDGES_REC_REWARD] = (double)reward[e];
    r[BRIDGES_REC_LIN] = (double)lin_reward[e];
    r[BRIDGES_REC_DONE] = (f[5] | f[6]) ? 1.0 : 0.0;                     // done | no_actions
    r[BRIDGES_REC_STABLE_N] = f[1] ? 1.0 : 0.0;
    valid[e] = f[0] != 0;
}

// Per-episode statistics of the vectorised loop: log_episode of the reference (successor_dqn.py:479-499) folded over the
// lock-step records of every env, before they are gathered (env identity still holds).  Per valid env e, with i = the record's
// step index (n_blocks of s: every episode starts from the empty assembly and places one block per env-step):
//   i == 0 restarts run[e];  run[e] += gpow[i] * (reward, lin_reward)  as float32 products and left-to-right float32 sums, no
//   fused multiply-add (the reference's sum(gamma ** i * t.reward ...) over float32 tensors);  at done the episode's
//   (1, run, i + 1, stable(s'), reward == n_targets) is added to row cls[e] of out [n_classes, 8] unless count_first_only and
//   counted[e] > 0, then counted[e]++.
// cls is the class the episode was played under (per-span / per-height statistics of a task family), snapshotted before the step
// that redraws it; a cls outside [0, n_classes) is counted in no row, run and counted advance as ever.  MAX_CLASSES = 1 is the
// fold without classes: the class is the constant 0, cls is not read and out is one row.
// ONE workgroup: thread t walks envs t, t + 256, ... and keeps one partial per (class, slot) in registers -- the class loop is
// unrolled, a partial takes the add only for its own class, so the order of the adds within a class does not depend on
// MAX_CLASSES; the classes go one after the other through a fixed-order LDS tree in f64 and thread k adds slot k to out.  No
// atomics, so two runs on the same inputs give the same bits, and one class with cls all zero gives the bits of MAX_CLASSES = 1.
constexpr int EPISODE_STATS_THREADS = 256;
constexpr int EPISODE_STATS_SLOTS = 8;        // episodes, sum reward, sum lin_reward, sum num_steps, sum stable, sum success, 2 spare
constexpr int EPISODE_STATS_USED = 6;         // slots 6 and 7 stay 0
constexpr int EPISODE_STATS_MAX_CLASSES = 8;

template <int MAX_CLASSES>
__global__ __launch_bounds__(EPISODE_STATS_THREADS) void k_episode_stats(
        int E, int K, const double* __restrict__ rec, const uint8_t* __restrict__ valid, const float* __restrict__ gpow, int n_targets,
        int count_first_only, const int32_t* __restrict__ cls, int n_classes, float* __restrict__ run, int32_t* __restrict__ counted,
        double* __restrict__ out) {
    __shared__ double part[EPISODE_STATS_SLOTS][EPISODE_STATS_THREADS];
    const int t = threadIdx.x;
    double acc[MAX_CLASSES][EPISODE_STATS_USED];
#pragma unroll
    for (int c = 0; c < MAX_CLASSES; ++c)
#pragma unroll
        for (int k = 0; k < EPISODE_STATS_USED; ++k) acc[c][k] = 0.0;
    for (int e = t; e < E; e += EPISODE_STATS_THREADS) {
        if (!valid[e]) continue;
        const double* r = rec + (size_t)e * BRIDGES_REC_WIDTH;
        const int i = (int)r[BRIDGES_REC_NB];
        const int gi = i < 0 ? 0 : (i < K ? i : K - 1);                    // bounds only: a record's step index is < K
        const float reward = (float)r[BRIDGES_REC_REWARD];                 // float32 values stored exactly as float64
        const float lin = (float)r[BRIDGES_REC_LIN];
        float s0 = i == 0 ? 0.f : run[2 * e];
        float s1 = i == 0 ? 0.f : run[2 * e + 1];
        s0 = __fadd_rn(s0, __fmul_rn(gpow[gi], reward));
        s1 = __fadd_rn(s1, __fmul_rn(gpow[gi], lin));
        run[2 * e] = s0;
        run[2 * e + 1] = s1;
        if (r[BRIDGES_REC_DONE] > 0.5) {
            const int32_t cnt = counted[e];
            if (!(count_first_only && cnt > 0)) {
                const int ce = MAX_CLASSES > 1 ? cls[e] : 0;
                const double v[EPISODE_STATS_USED] = {1.0, (double)s0, (double)s1, (double)(i + 1),
                                                      r[BRIDGES_REC_STABLE_N] > 0.5 ? 1.0 : 0.0,
                                                      reward == (float)n_targets ? 1.0 : 0.0};
#pragma unroll
                for (int c = 0; c < MAX_CLASSES; ++c)
#pragma unroll
                    for (int k = 0; k < EPISODE_STATS_USED; ++k) acc[c][k] = ce == c ? acc[c][k] + v[k] : acc[c][k];
            }
            counted[e] = cnt + 1;
        }
    }
#pragma unroll
    for (int c = 0; c < MAX_CLASSES; ++c) {
        if (MAX_CLASSES > 1 && c >= n_classes) break;   // uniform: every thread sees the same n_classes
#pragma unroll
        for (int k = 0; k < EPISODE_STATS_SLOTS; ++k) part[k][t] = k < EPISODE_STATS_USED ? acc[c][k < EPISODE_STATS_USED ? k : 0] : 0.0;
        __syncthreads();
        for (int s = EPISODE_STATS_THREADS / 2; s > 0; s >>= 1) {
            if (t < s) {
#pragma unroll
                for (int k = 0; k < EPISODE_STATS_SLOTS; ++k) part[k][t] += part[k][t + s];
            }
            __syncthreads();
        }
        if (t < EPISODE_STATS_SLOTS) out[c * EPISODE_STATS_SLOTS + t] += part[t][0];
        __syncthreads();                            // the next class reuses the tree
    }
}

// One body for k_replay_unpack and k_replay_unpack_prev.  PREV loads the state s the transition was taken IN: the block list as
// stored (no action block, no occupancy update), n_blocks = NB, the candidate count of the free faces of s, and both ranges cover
// s; the scalar outputs are the same.
template <bool PREV>
__device__ __forceinline__ void replay_unpack_body(int E, int n_rec, int K, const double* __restrict__ rec,
                                                   const int32_t* __restrict__ shape_faces, int n_shapes, int n_groups, int n_ground, int n_off,
                                                   int32_t* __restrict__ n_blocks, int32_t* __restrict__ blk_shape,
                                                   double* __restrict__ blk_pose, uint8_t* __restrict__ blk_occ,
                                                   int32_t* __restrict__ n_cand, int32_t* __restrict__ ranges_next,
                                                   int32_t* __restrict__ ranges_prev, float* __restrict__ lin,
                                                   float* __restrict__ stable_s, uint8_t* __restrict__ done,
                                                   uint8_t* __restrict__ stable_n) {
    const int e = blockIdx.x, k = threadIdx.x;
    if (e >= E) return;
    const double* r = rec + (size_t)(e < n_rec ? e : 0) * BRIDGES_REC_WIDTH;     // padding envs repeat the first record
    const int nb = (int)r[BRIDGES_REC_NB];
    const int slot = nb < K - 1 ? nb : K - 1;
    const int tb = (int)r[BRIDGES_REC_ATB];
    int free_faces = 0;
    if (k < K) {
        int shape = (int)r[BRIDGES_REC_SHAPE + k];
        int occ = (int)r[BRIDGES_REC_OCC + k] & 255;
        double p[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = r[BRIDGES_REC_POSE + 4 * k + j];
        if (!PREV && k == slot) {                                          // the action block
            shape = (int)r[BRIDGES_REC_ASHAPE];
            occ = (1 << (int)r[BRIDGES_REC_AFACE]) & 255;
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = r[BRIDGES_REC_APOSE + j];
        }
        if (!PREV && tb >= 0 && k == tb) occ |= (1 << (int)r[BRIDGES_REC_ATF]) & 255;   // the face it was put on
        blk_shape[(size_t)e * K + k] = shape;
        blk_occ[(size_t)e * K + k] = (uint8_t)occ;
#pragma unroll
        for (int j = 0; j < 4; ++j) blk_pose[((size_t)e * K + k) * 4 + j] = p[j];
        if ((PREV ? k < nb : k <= nb) && k < K) free_faces = shape_faces[shape < 0 ? 0 : (shape < n_shapes ? shape : n_shapes - 1)] - __builtin_popcount(occ & ((1 << BRIDGES_MAX_VERTS) - 1));
    }
    int nfree = free_faces;                                                // lanes >= K hold 0
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) nfree += __shfl_xor(nfree, m);
    if (k == 0) {
        n_blocks[e] = PREV ? nb : nb + 1;
        n_cand[e] = n_groups * (n_ground + nfree * n_off);     // raw count: bridges_env_refresh clamps to the env's a_max and flags it
        ranges_next[2 * e] = e * K;
        ranges_next[2 * e + 1] = PREV ? e * K + nb : e * K + nb + 1;
        ranges_prev[2 * e] = e * K;
        ranges_prev[2 * e + 1] = e * K + nb;
        lin[e] = (float)r[BRIDGES_REC_LIN];
        stable_s[e] = (float)r[BRIDGES_REC_STABLE_S];
        done[e] = r[BRIDGES_REC_DONE] > 0.5;
        stable_n[e] = r[BRIDGES_REC_STABLE_N] > 0.5;
    }
}

__global__ __launch_bounds__(64) void k_replay_unpack(int E, int n_rec, int K, const double* __restrict__ rec,
                                                      const int32_t* __restrict__ shape_faces, int n_shapes, int n_groups, int n_ground, int n_off,
                                                      int32_t* __restrict__ n_blocks, int32_t* __restrict__ blk_shape,
                                                      double* __restrict__ blk_pose, uint8_t* __restrict__ blk_occ,
                                                      int32_t* __restrict__ n_cand, int32_t* __restrict__ ranges_next,
                                                      int32_t* __restrict__ ranges_prev, float* __restrict__ lin,
                                                      float* __restrict__ stable_s, uint8_t* __restrict__ done,
                                                      uint8_t* __restrict__ stable_n) {
    replay_unpack_body<false>(E, n_rec, K, rec, shape_faces, n_shapes, n_groups, n_ground, n_off, n_blocks, blk_shape, blk_pose, blk_occ, n_cand,
                              ranges_next, ranges_prev, lin, stable_s, done, stable_n);
}

__global__ __launch_bounds__(64) void k_replay_unpack_prev(int E, int n_rec, int K, const double* __restrict__ rec,
                                                           const int32_t* __restrict__ shape_faces, int n_shapes, int n_groups, int n_ground, int n_off,
                                                           int32_t* __restrict__ n_blocks, int32_t* __restrict__ blk_shape,
                                                           double* __restrict__ blk_pose, uint8_t* __restrict__ blk_occ,
                                                           int32_t* __restrict__ n_cand, int32_t* __restrict__ ranges_next,
                                                           int32_t* __restrict__ ranges_prev, float* __restrict__ lin,
                                                           float* __restrict__ stable_s, uint8_t* __restrict__ done,
                                                           uint8_t* __restrict__ stable_n) {
    replay_unpack_body<true>(E, n_rec, K, rec, shape_faces, n_shapes, n_groups, n_ground, n_off, n_blocks, blk_shape, blk_pose, blk_occ, n_cand,
                              ranges_next, ranges_prev, lin, stable_s, done, stable_n);
}

}  // namespace bridges
