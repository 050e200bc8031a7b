// Munchausen targets (bridges_soft_value, bridges_action_row; the rule stands in include/bridges_hip.h).
#include "bridges_device.h"

namespace bridges {

// ---------------------------------------------------------------------------------------------------------------
// The log-sum-exp value of a segment of q and the scaled log-policy of one of its rows:
//   V = m + T log Z,  Z = sum_j w_j,  w_j = boltzmann_weight(q_j, m, T)  (k_boltzmann_select's weights, by its very function),
//   L = T ln pi(a) = (q_a - m) - T log Z,  bonus = alpha * max(L, clip_lo).
// One wave owns a segment, a 256-lane workgroup holds four (boltzmann_select_body's layout); lo and hi are made scalar, so every
// lane reaches every cross-lane step.  Pass 1: the largest eligible q, lane-strided, wave_max_d.  REL: segment_spread with the
// identity combine, then T = relative_temperature().  Pass 2: Z, lane-strided partial sums through wave_sum_d.  Lane 0 writes
// every output.  float64 throughout, one rounding to float32 per output; no LDS, no scratch, no atomics, a fixed order of
// additions: the same inputs give the same bits.
template <bool REL>
__device__ __forceinline__ void soft_value_body(int n, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                const float* __restrict__ q, float temperature, float spread_floor,
                                                const int32_t* __restrict__ taken_row, float alpha, float clip_lo,
                                                float* __restrict__ value, float* __restrict__ tlogp, float* __restrict__ bonus,
                                                uint8_t* __restrict__ miss, double* __restrict__ temp_out) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    if (i >= n) return;                                  // wave-uniform: i is the same in all 64 lanes
    const int lo = __builtin_amdgcn_readfirstlane(seg_lo[i]), hi = __builtin_amdgcn_readfirstlane(seg_hi[i]);
    // pass 1: the largest eligible q (-inf: nothing is eligible; that includes the empty segment)
    double mx = -(double)INFINITY;
    for (int j = lo + lane; j < hi; j += WAVE) {
        const float v = q[j];
        if (v == v && (double)v > mx) mx = (double)v;
    }
    const double m = wave_max_d(mx);
    const bool any = m != -(double)INFINITY;             // uniform
    double T = (double)temperature;
    if (REL) {
        double spread = 0.0;                             // (nothing eligible: no row is finite either)
        if (any) spread = segment_spread<WAVE>(q, lo, hi, lane, [](double v, int) { return v; });
        T = relative_temperature(temperature, spread, spread_floor);
    }
    double tlz = 0.0;                                    // T log Z (m = +inf: T log of the number of +inf rows)
    if (any) {
        // pass 2: Z
        double z = 0.0;
        for (int j = lo + lane; j < hi; j += WAVE) z += boltzmann_weight(q[j], m, T);
        tlz = T * log(wave_sum_d(z));
    }
    if (lane == 0) {
        value[i] = any ? (float)(m + tlz) : -INFINITY;   // (m = +inf: +inf)
        if (REL) temp_out[i] = T;
        if (taken_row) {
            const int a = taken_row[i];
            bool hit = false;
            double L = 0.0;
            if (any && a >= lo && a < hi) {              // (the sentinel 0x7fffffff is below no hi)
                const float qa = q[a];
                if (qa == qa && qa != -INFINITY) {
                    hit = true;
                    if (m == (double)INFINITY) L = qa == INFINITY ? 0.0 - tlz : -(double)INFINITY;
                    else L = fmin(((double)qa - m) - tlz, 0.0);
                }
            }
            tlogp[i] = (float)L;
            // (+ 0.0: a product of 0 and a negative factor is -0.0; the bonus of such a row is +0.0)
            bonus[i] = hit ? (float)((double)alpha * fmax(L, (double)clip_lo) + 0.0) : 0.f;
            miss[i] = hit ? 0 : 1;
        }
    }
}

__global__ __launch_bounds__(256) void k_soft_value(int n, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                    const float* __restrict__ q, float temperature,
                                                    const int32_t* __restrict__ taken_row, float alpha, float clip_lo,
                                                    float* __restrict__ value, float* __restrict__ tlogp, float* __restrict__ bonus,
                                                    uint8_t* __restrict__ miss) {
    soft_value_body<false>(n, seg_lo, seg_hi, q, temperature, 0.f, taken_row, alpha, clip_lo, value, tlogp, bonus, miss, nullptr);
}

__global__ __launch_bounds__(256) void k_soft_value_rel(int n, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                        const float* __restrict__ q, float temperature, float spread_floor,
                                                        const int32_t* __restrict__ taken_row, float alpha, float clip_lo,
                                                        float* __restrict__ value, float* __restrict__ tlogp,
                                                        float* __restrict__ bonus, uint8_t* __restrict__ miss,
                                                        double* __restrict__ temp_out) {
    soft_value_body<true>(n, seg_lo, seg_hi, q, temperature, spread_floor, taken_row, alpha, clip_lo, value, tlogp, bonus, miss,
                          temp_out);
}

// ---------------------------------------------------------------------------------------------------------------
// The row of a rebuilt candidate set that holds the action a record took: the first row j of the segment whose candidate
// c = idx[j] has the record's descriptor (ATB, ATF, ASHAPE, AFACE) and the record's four pose words, compared as 64-bit
// patterns (ground positions and offsets share a descriptor: the pose decides; -0.0 is not 0.0).  One wave per transition, four
// per workgroup; lane j takes row base + j of a chunk of 64: idx, the 16-byte descriptor, the 32-byte pose; the first match
// comes off wave_min_i, and the walk stops at the first chunk that holds one.  No atomics, one store per transition.
__global__ __launch_bounds__(256) void k_action_row(int n, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                    const int64_t* __restrict__ idx, const int32_t* __restrict__ cand_desc,
                                                    const double* __restrict__ cand_pose, const double* __restrict__ rec,
                                                    int64_t rec_stride, int32_t* __restrict__ row) {
    constexpr int NONE = 0x7fffffff;
    const int lane = threadIdx.x & (WAVE - 1);
    const int i = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
    if (i >= n) return;                                  // wave-uniform
    const int lo = __builtin_amdgcn_readfirstlane(seg_lo[i]), hi = __builtin_amdgcn_readfirstlane(seg_hi[i]);
    const double* r = rec + (int64_t)i * rec_stride;
    // (the record holds the descriptor's integers exactly as float64: compared as such, no conversion of a word that is none)
    const double d0 = r[BRIDGES_REC_ATB], d1 = r[BRIDGES_REC_ATF], d2 = r[BRIDGES_REC_ASHAPE], d3 = r[BRIDGES_REC_AFACE];
    const uint64_t* rp = reinterpret_cast<const uint64_t*>(r + BRIDGES_REC_APOSE);
    const uint64_t p0 = rp[0], p1 = rp[1], p2 = rp[2], p3 = rp[3];
    int found = NONE;
    for (int base = lo < 0 ? 0 : lo; base < hi; base += WAVE) {
        const int j = base + lane;
        bool match = false;
        if (j < hi) {
            const int64_t c = idx[j];
            const int4 d = *reinterpret_cast<const int4*>(cand_desc + c * 4);
            const uint64_t* cp = reinterpret_cast<const uint64_t*>(cand_pose + c * 4);
            match = (double)d.x == d0 && (double)d.y == d1 && (double)d.z == d2 && (double)d.w == d3 &&
                    cp[0] == p0 && cp[1] == p1 && cp[2] == p2 && cp[3] == p3;
        }
        found = wave_min_i(match ? j : NONE);
        if (found != NONE) break;                        // wave-uniform: wave_min_i returns a scalar
    }
    if (lane == 0) row[i] = found;
}

}  // namespace bridges
