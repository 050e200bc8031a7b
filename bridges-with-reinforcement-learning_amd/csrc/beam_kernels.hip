// bridges_beam_select: the top-B candidates of every group of B beams (include/bridges_hip.h has the rule).
//
// E = G * B envs; group g owns envs gB .. gB + B - 1, and rows seg_lo[e] .. seg_hi[e] of q / idx are env e's (its
// representative's, with rep).  A candidate is a pair (live env e, row j of e) whose q is neither NaN nor -inf and whose score
//   S = ret[e] + disc[e] * (double)q[j]            (two binary64 operations; the library is compiled without contraction)
// is not NaN.  Candidates are ordered by S descending, then q descending, then env ascending, then row ascending: a strict
// total order, so "the i-th candidate" is well defined and no reduction order can change it.
//
// One workgroup per group, B rounds.  Round i finds the best candidate that comes strictly AFTER round i - 1's pick in the
// order, so nothing has to be marked as taken: every lane scans its share of the group's rows, the waves reduce by shuffles,
// the workgroup through LDS.  No atomics, no scratch, the same bits on every call.  The rows of a group are read B times; they
// are a few thousand floats and stay in cache.
#include "bridges_device.h"

namespace bridges {

#define BEAM_THREADS 256
#define BEAM_MAX_WIDTH 16

struct BeamKey {            // one candidate; env < 0: none
    double S;
    float q;
    int env, row;
};

// a comes before b in the order (both candidates)
__device__ __forceinline__ bool beam_before(const BeamKey& a, const BeamKey& b) {
    if (a.S != b.S) return a.S > b.S;
    if (a.q != b.q) return a.q > b.q;
    if (a.env != b.env) return a.env < b.env;
    return a.row < b.row;
}

__device__ __forceinline__ void beam_take(BeamKey& best, const BeamKey& k) {
    if (k.env >= 0 && (best.env < 0 || beam_before(k, best))) best = k;
}

__global__ __launch_bounds__(BEAM_THREADS) void k_beam_select(int E, int B, int n_rows, const int32_t* __restrict__ seg_lo,
                                                              const int32_t* __restrict__ seg_hi, const float* __restrict__ q,
                                                              const int64_t* __restrict__ idx, const int32_t* __restrict__ cand_offset,
                                                              const int32_t* __restrict__ rep, const uint8_t* __restrict__ live,
                                                              const double* __restrict__ ret, const double* __restrict__ disc,
                                                              int32_t* __restrict__ src, int64_t* __restrict__ sel_compact,
                                                              int32_t* __restrict__ sel_index, float* __restrict__ q_sel,
                                                              double* __restrict__ score, uint8_t* __restrict__ live_out) {
    __shared__ BeamKey part[BEAM_THREADS / WAVE];
    __shared__ BeamKey prev_s;
    __shared__ int lo_s[BEAM_MAX_WIDTH], hi_s[BEAM_MAX_WIDTH];
    __shared__ double ret_s[BEAM_MAX_WIDTH], disc_s[BEAM_MAX_WIDTH];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int e0 = blockIdx.x * B;
    if (e0 + B > E) return;
    if (t < B) {
        const int e = e0 + t;
        int lo = seg_lo[e], hi = seg_hi[e];
        if (lo < 0) lo = 0;
        if (hi > n_rows) hi = n_rows;
        if (!live[e]) hi = lo;                              // a dead beam has no candidates
        lo_s[t] = lo; hi_s[t] = hi;
        ret_s[t] = ret[e]; disc_s[t] = disc[e];
    }
    if (t == 0) prev_s.env = -1;
    __syncthreads();
    for (int round = 0; round < B; ++round) {
        const BeamKey prev = prev_s;
        BeamKey best;
        best.S = 0.0; best.q = 0.f; best.env = -1; best.row = 0;
        if (round == 0 || prev.env >= 0) {                  // (nothing was left in the round before: nothing is left now)
            for (int b = 0; b < B; ++b) {
                const double r = ret_s[b], d = disc_s[b];
                for (int j = lo_s[b] + t; j < hi_s[b]; j += BEAM_THREADS) {
                    const float v = q[j];
                    if (v != v || v == -INFINITY) continue;
                    BeamKey k;
                    k.S = r + d * (double)v;
                    if (k.S != k.S) continue;
                    k.q = v; k.env = e0 + b; k.row = j;
                    if (prev.env >= 0 && !beam_before(prev, k)) continue;     // taken already, or the previous pick itself
                    beam_take(best, k);
                }
            }
        }
#pragma unroll
        for (int m = 1; m < WAVE; m <<= 1) {
            BeamKey o;
            o.S = __shfl_xor(best.S, m); o.q = __shfl_xor(best.q, m); o.env = __shfl_xor(best.env, m); o.row = __shfl_xor(best.row, m);
            beam_take(best, o);
        }
        if (lane == 0) part[wv] = best;
        __syncthreads();
        if (t == 0) {
            BeamKey w = part[0];
            for (int k = 1; k < BEAM_THREADS / WAVE; ++k) beam_take(w, part[k]);
            prev_s = w;
            const int slot = e0 + round;
            if (w.env >= 0) {
                const int64_t c = idx[w.row];
                int owner = rep ? rep[w.env] : w.env;
                if (owner < 0 || owner >= E) owner = w.env;
                const int64_t rel = c - (int64_t)cand_offset[owner];
                src[slot] = w.env; sel_compact[slot] = c; sel_index[slot] = rel > 0 ? (int32_t)rel : 0;
                q_sel[slot] = w.q; score[slot] = w.S; live_out[slot] = 1;
            } else {
                src[slot] = slot; sel_compact[slot] = 0; sel_index[slot] = 0;
                q_sel[slot] = 0.f; score[slot] = -INFINITY; live_out[slot] = 0;
            }
        }
        __syncthreads();
    }
}

}  // namespace bridges
