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

// bridges_beam_merge: the beams of a group that hold the same structure, placed in whatever order (include/bridges_hip.h has the
// rule).  A live slot is a tuple of five 64-bit words -- shape id | occupancy << 32, then the four pose bit patterns --, an env's
// key is (nb, targets_left, [the tuple of slot nb - 1], the sorted multiset of its tuples), and two live envs of a group are
// equivalent iff their keys agree word for word.
//
// One workgroup per group, a wave per env (the waves take the group's envs in turn).  Pass 1: lane i < nb holds slot i's tuple and
// counts the slots that come before it in the lexicographic order of the words, ties by slot index -- a total order, so the counts
// are a permutation --, and writes its tuple to that place of the env's sorted row in LDS (K <= 64: one lane per slot; rows of 40
// bytes per lane: no bank conflicts).  Pass 2, after the barrier: the env's wave holds its sorted row against that of every other
// live env of the group, one lane per slot and one ballot per pair, and keeps the first equivalent env by (ret descending, env
// ascending).  Nothing is accepted on a hash; no atomics, no scratch, every output written once.
#define BEAM_TUPLE_WORDS 5
#define BEAM_MAX_SLOTS 64

struct BeamTuple {
    uint64_t w[BEAM_TUPLE_WORDS];
};

__device__ __forceinline__ bool beam_tuple_less(const BeamTuple& a, const BeamTuple& b) {
#pragma unroll
    for (int k = 0; k < BEAM_TUPLE_WORDS; ++k)
        if (a.w[k] != b.w[k]) return a.w[k] < b.w[k];
    return false;
}

__device__ __forceinline__ bool beam_tuple_equal(const BeamTuple& a, const BeamTuple& b) {
    bool same = true;
#pragma unroll
    for (int k = 0; k < BEAM_TUPLE_WORDS; ++k) same = same && a.w[k] == b.w[k];
    return same;
}

// ret a ranks strictly above ret b: a binary64 >, a NaN below every number (two NaNs tie)
__device__ __forceinline__ bool beam_ret_above(double a, double b) {
    if (a != a) return false;
    if (b != b) return true;
    return a > b;
}

__global__ __launch_bounds__(BEAM_THREADS) void k_beam_merge(int E, int B, int K, const int32_t* __restrict__ n_blocks,
                                                             const int32_t* __restrict__ blk_shape, const double* __restrict__ blk_pose,
                                                             const uint8_t* __restrict__ blk_occ, const int32_t* __restrict__ targets_left,
                                                             const uint8_t* __restrict__ live, const double* __restrict__ ret, int key_last,
                                                             int32_t* __restrict__ rep, uint8_t* __restrict__ live_out,
                                                             int32_t* __restrict__ n_merged) {
    __shared__ BeamTuple sorted_s[BEAM_MAX_WIDTH][BEAM_MAX_SLOTS];
    __shared__ BeamTuple last_s[BEAM_MAX_WIDTH];
    __shared__ int nb_s[BEAM_MAX_WIDTH], tl_s[BEAM_MAX_WIDTH], live_s[BEAM_MAX_WIDTH], closed_s[BEAM_MAX_WIDTH];
    __shared__ double ret_s[BEAM_MAX_WIDTH];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int e0 = blockIdx.x * B;
    if (e0 + B > E) return;
    for (int b = wv; b < B; b += BEAM_THREADS / WAVE) {      // pass 1: env e0 + b's tuples, sorted, into LDS
        const int e = e0 + b;
        const int alive = live[e] != 0;
        int nb = n_blocks[e];
        nb = nb < 0 ? 0 : (nb > K ? K : nb);
        if (lane == 0) { nb_s[b] = nb; tl_s[b] = targets_left[e]; live_s[b] = alive; ret_s[b] = ret[e]; }
        if (!alive) continue;                                // (wave-uniform) a dead env matches nothing
        BeamTuple mine;
#pragma unroll
        for (int k = 0; k < BEAM_TUPLE_WORDS; ++k) mine.w[k] = 0ull;
        if (lane < nb) {
            const size_t s = (size_t)e * K + lane;
            const uint64_t* p = reinterpret_cast<const uint64_t*>(blk_pose + s * 4);
            mine.w[0] = (uint64_t)(uint32_t)blk_shape[s] | ((uint64_t)blk_occ[s] << 32);
            mine.w[1] = p[0]; mine.w[2] = p[1]; mine.w[3] = p[2]; mine.w[4] = p[3];
        }
        int before = 0;
        for (int j = 0; j < nb; ++j) {                       // (nb is wave-uniform: every lane takes part in the shuffles)
            BeamTuple o;
#pragma unroll
            for (int k = 0; k < BEAM_TUPLE_WORDS; ++k) o.w[k] = __shfl(mine.w[k], j);
            before += (beam_tuple_less(o, mine) || (j < lane && beam_tuple_equal(o, mine))) ? 1 : 0;
        }
        if (lane < nb) {
            sorted_s[b][before] = mine;                      // before < nb: it counts slots other than this one
            if (lane == nb - 1) last_s[b] = mine;
        }
    }
    __syncthreads();
    for (int b = wv; b < B; b += BEAM_THREADS / WAVE) {      // pass 2: the representative of env e0 + b
        const int nb = nb_s[b];
        int best = b;
        if (live_s[b]) {
            BeamTuple mine;
            if (lane < nb) mine = sorted_s[b][lane];
            for (int o = 0; o < B; ++o) {
                if (o == b || !live_s[o] || nb_s[o] != nb || tl_s[o] != tl_s[b]) continue;           // (wave-uniform)
                bool differs = lane < nb && !beam_tuple_equal(mine, sorted_s[o][lane]);
                if (key_last && nb > 0 && lane == 0) differs = differs || !beam_tuple_equal(last_s[b], last_s[o]);
                if (__ballot(differs) != 0ull) continue;
                // o is of b's class: it takes the place of best if it comes before it by (ret descending, env ascending)
                if (beam_ret_above(ret_s[o], ret_s[best]) || (!beam_ret_above(ret_s[best], ret_s[o]) && o < best)) best = o;
            }
        }
        if (lane == 0) {
            const int e = e0 + b;
            rep[e] = e0 + best;
            live_out[e] = (live_s[b] && best == b) ? 1 : 0;
            closed_s[b] = (live_s[b] && best != b) ? 1 : 0;
        }
    }
    __syncthreads();
    if (t == 0) {
        int n = 0;
        for (int b = 0; b < B; ++b) n += closed_s[b];
        n_merged[blockIdx.x] = n;
    }
}

}  // namespace bridges
