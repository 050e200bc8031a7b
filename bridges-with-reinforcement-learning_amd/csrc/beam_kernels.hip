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

// bridges_particle_select: the sampled sibling of bridges_beam_select (include/bridges_hip.h has the rule).  Same layout; a live env
// with an eligible row (q neither NaN nor -inf) and a value
//   S_e = ret[e] + disc[e] * (double)(the env's largest eligible q)      (two binary64 operations, as the beam's score)
// that is neither NaN nor -inf is a PARENT.  The parents of a group weigh W_p = exp((S_p - max S) / T_r); slot k takes, by systematic
// resampling at (u_res[g] + k) / B of the total, the first parent whose inclusive prefix sum in env order exceeds the target
// (strictly), and draws one of that PARENT's rows by the rule of bridges_boltzmann_select at `temperature` with u_act[gB + k].  With
// elite != 0 slot 0 is afterwards given the first best parent and that parent's first maximum of q.
//
// One workgroup per group, three phases with a barrier between them.  (1) A wave per env (the four waves take the group's envs in
// turn): the largest eligible q (lane-strided, DPP tree), S and the clamped row range into LDS.  (2) One lane: the B weights, their
// prefix sums added one by one in env order -- at most 16 terms, so the order is the rule's own and costs nothing --, ess, and the
// parent of every slot.  (3) A wave per slot: the total and the scan of k_boltzmann_select (64 rows at a time, chunks in order) over
// the parent's rows, with boltzmann_weight of dqn_kernels.hip and the maximum of phase 1; the draw's loop is written again here so
// that k_boltzmann_select's code stays as it is.  No atomics, no scratch, every output word written once, the same bits on every call.
__global__ __launch_bounds__(BEAM_THREADS) void k_particle_select(
    int E, int B, int n_rows, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi, const float* __restrict__ q,
    const int64_t* __restrict__ idx, const int32_t* __restrict__ cand_offset, const int32_t* __restrict__ rep,
    const uint8_t* __restrict__ live, const double* __restrict__ ret, const double* __restrict__ disc, const float* __restrict__ u_act,
    const float* __restrict__ u_res, float temperature, float resample_temperature, int elite, int32_t* __restrict__ src,
    int64_t* __restrict__ sel_compact, int32_t* __restrict__ sel_index, float* __restrict__ q_sel, double* __restrict__ score,
    uint8_t* __restrict__ live_out, float* __restrict__ p_sel, double* __restrict__ ess) {
    constexpr int NONE = 0x7fffffff;
    __shared__ int lo_s[BEAM_MAX_WIDTH], hi_s[BEAM_MAX_WIDTH], parent_s[BEAM_MAX_WIDTH], slot_parent_s[BEAM_MAX_WIDTH];
    __shared__ double ret_s[BEAM_MAX_WIDTH], disc_s[BEAM_MAX_WIDTH], max_s[BEAM_MAX_WIDTH], S_s[BEAM_MAX_WIDTH];
    __shared__ double W_s[BEAM_MAX_WIDTH], C_s[BEAM_MAX_WIDTH];
    const int t = threadIdx.x, lane = t & (WAVE - 1);
    const int wv = __builtin_amdgcn_readfirstlane(t / WAVE);
    const int g = blockIdx.x, e0 = g * B;
    if (e0 + B > E) return;
    for (int b = wv; b < B; b += BEAM_THREADS / WAVE) {      // phase 1: env e0 + b's range, largest eligible q and value
        const int e = e0 + b;
        int lo = __builtin_amdgcn_readfirstlane(seg_lo[e]), hi = __builtin_amdgcn_readfirstlane(seg_hi[e]);
        if (lo < 0) lo = 0;
        if (hi > n_rows) hi = n_rows;
        double mx = -INFINITY;
        for (int j = lo + lane; j < hi; j += WAVE) {
            const float v = q[j];
            if (v == v && (double)v > mx) mx = (double)v;
        }
        const double m = wave_max_d(mx);                     // -inf: no eligible row
        if (lane == 0) {
            const double r = ret[e], d = disc[e];
            const double S = r + d * m;
            lo_s[b] = lo; hi_s[b] = hi; ret_s[b] = r; disc_s[b] = d; max_s[b] = m; S_s[b] = S;
            parent_s[b] = (live[e] && m != -(double)INFINITY && S == S && S != -(double)INFINITY) ? 1 : 0;
        }
    }
    __syncthreads();
    if (t == 0) {                                            // phase 2: weights, prefix sums, the parent of every slot
        const double Tr = (double)resample_temperature;
        double M = -INFINITY;
        int n_par = 0, best = -1;
        for (int b = 0; b < B; ++b) {
            if (!parent_s[b]) continue;
            ++n_par;
            if (best < 0 || S_s[b] > M) { M = S_s[b]; best = b; }               // the first parent of maximal S
        }
        double run = 0.0, sq = 0.0;
        int last_pos = -1;
        for (int b = 0; b < B; ++b) {
            double w = 0.0;
            if (parent_s[b]) {
                if (Tr == (double)INFINITY) w = 1.0;
                else if (M == (double)INFINITY) w = S_s[b] == (double)INFINITY ? 1.0 : 0.0;
                else w = exp((S_s[b] - M) / Tr);
            }
            run += w; sq += w * w;
            W_s[b] = w; C_s[b] = run;
            if (w > 0.0) last_pos = b;
        }
        const double total = run;
        ess[g] = n_par ? total * total / sq : 0.0;
        for (int k = 0; k < B; ++k) {
            int p = -1;
            if (n_par) {
                const double target = ((double)u_res[g] + (double)k) / (double)B * total;
                p = last_pos;
                for (int b = B - 1; b >= 0; --b)
                    if (W_s[b] > 0.0 && C_s[b] > target) p = b;                 // ends on the first such b
                if (elite && k == 0) p = best;
            }
            slot_parent_s[k] = p;
        }
    }
    __syncthreads();
    for (int k = wv; k < B; k += BEAM_THREADS / WAVE) {      // phase 3: slot k's row of its parent
        const int slot = e0 + k;
        const int p = slot_parent_s[k];                      // wave-uniform
        if (p < 0) {
            if (lane == 0) {
                src[slot] = slot; sel_compact[slot] = 0; sel_index[slot] = 0;
                q_sel[slot] = 0.f; score[slot] = -INFINITY; live_out[slot] = 0; p_sel[slot] = 0.f;
            }
            continue;
        }
        const int lo = lo_s[p], hi = hi_s[p];
        const double m = max_s[p], T = (double)temperature;
        int row;
        double prob;
        if (elite && k == 0) {
            int fm = NONE;
            for (int j = lo + lane; j < hi; j += WAVE)
                if (fm == NONE && (double)q[j] == m) fm = j;
            row = wave_min_i(fm);
            prob = 1.0;
        } else {
            // k_boltzmann_select's passes 2 and 3 over the parent's rows
            double total = 0.0;
            for (int base = lo; base < hi; base += WAVE) {
                const int j = base + lane;
                total += wave_sum_d(boltzmann_weight(j < hi ? q[j] : -INFINITY, m, T));
            }
            const double target = (double)u_act[slot] * total;
            double carry = 0.0;
            int last_pos = -1, found = NONE;
            for (int base = lo; base < hi; base += WAVE) {
                const int j = base + lane;
                const double w = boltzmann_weight(j < hi ? q[j] : -INFINITY, m, T);
                double incl = w;
#pragma unroll
                for (int s = 1; s < WAVE; s <<= 1) {
                    const double up = __shfl_up(incl, s, WAVE);
                    if (lane >= s) incl += up;
                }
                if (w > 0.0) last_pos = j;
                found = wave_min_i((j < hi && carry + incl > target) ? j : NONE);
                if (found != NONE) break;                    // wave-uniform
                carry += readlane_d(incl, WAVE - 1);
            }
            if (found == NONE) found = -wave_min_i(-last_pos);                 // (a parent has a row of weight 1: last_pos >= lo)
            row = found;
            prob = boltzmann_weight(q[row], m, T) / total;
        }
        if (lane == 0) {
            const int pe = e0 + p;
            const float v = q[row];
            const int64_t c = idx[row];
            int owner = rep ? rep[pe] : pe;
            if (owner < 0 || owner >= E) owner = pe;
            const int64_t rel = c - (int64_t)cand_offset[owner];
            src[slot] = pe; sel_compact[slot] = c; sel_index[slot] = rel > 0 ? (int32_t)rel : 0;
            q_sel[slot] = v; score[slot] = ret_s[p] + disc_s[p] * (double)v; live_out[slot] = 1; p_sel[slot] = (float)prob;
        }
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

// bridges_beam_trace: the transition records of one finished beam per group, read back along the parent pointers of the search
// (include/bridges_hip.h has the rule).  Per depth t the search keeps rec [D, E, REC_WIDTH], valid [D, E] and parent [D, E] (the src
// of that depth's select); a group names the end (end_env, end_depth) of one episode, whose chain is e_{L-1} = end_env,
// e_{t-1} = parent[t][e_t].
//
// Two launches, one workgroup per group in both, no scratch:
//   k_beam_trace_check   the group's [D, B] slices of parent and valid go to LDS in parallel (at most 256 words each), one lane
//                        walks the chain there, status[g] = 1 for a broken chain.
//   k_beam_trace_rows    the same load and walk (a few dozen LDS reads: cheaper than a trip through memory for the chain); the
//                        group's row offset is the sum of the rows of the groups in front of it -- L of every group with an end and
//                        status 0, integers, so the order of the sum cannot matter --; lanes t < L fetch lin_t and stable_t of their
//                        chain member; lane t sums the return of start t in the fixed order of bridges_nstep_fold; then a wave per
//                        row, the lanes on consecutive doubles of it.
// The offsets cost G reads per workgroup (G is a number of tasks: tens to hundreds) and save the scan launch and its scratch.
// No atomics; every output word is written at most once; the same bits on every call.
static_assert(BRIDGES_REC_K * BEAM_MAX_WIDTH <= BEAM_THREADS, "a group's [D, B] slice is loaded by one lane per word");

struct BeamTraceArgs {
    const double* rec;
    const uint8_t* valid;
    const int32_t* parent;
    const int32_t* end_env;
    const int32_t* end_depth;
    const double* tail;
    double gamma, priority;
    int E, B, D, n_step, n_tail;
};

// The walk of group g in LDS: par_s / val_s [D * B] hold the group's slices (parent as given, row 0 unused), chain_s [D] receives
// e_t - gB.  -> L (0: nothing ended, or the chain is broken), broken set accordingly.  Called by one lane.
__device__ __forceinline__ int beam_trace_walk(const BeamTraceArgs& a, int g, const int* par_s, const uint8_t* val_s, int* chain_s,
                                               bool& broken) {
    const int B = a.B, e0 = g * B;
    const int ed = a.end_depth[g];
    broken = false;
    if (ed < 0) return 0;
    broken = true;
    if (ed >= a.D) return 0;
    const int ee = a.end_env[g];
    int b = (ee < e0 || ee >= e0 + B) ? -1 : ee - e0;
    for (int t = ed; t >= 0; --t) {
        if (b < 0 || b >= B || !val_s[t * B + b]) return 0;
        chain_s[t] = b;
        if (t > 0) {
            const int p = par_s[t * B + b];
            b = (p < e0 || p >= e0 + B) ? -1 : p - e0;
        }
    }
    broken = false;
    return ed + 1;
}

__device__ __forceinline__ void beam_trace_load(const BeamTraceArgs& a, int g, int* par_s, uint8_t* val_s) {
    const int i = threadIdx.x;                              // D * B <= BRIDGES_REC_K * BEAM_MAX_WIDTH = BEAM_THREADS
    if (i < a.D * a.B) {
        const int t = i / a.B, b = i % a.B;
        const size_t at = (size_t)t * a.E + (size_t)g * a.B + b;
        par_s[i] = t > 0 ? a.parent[at] : 0;                // row 0 of parent is never read
        val_s[i] = a.valid[at];
    }
}

__global__ __launch_bounds__(BEAM_THREADS) void k_beam_trace_check(BeamTraceArgs a, int32_t* __restrict__ status) {
    __shared__ int par_s[BEAM_THREADS];
    __shared__ uint8_t val_s[BEAM_THREADS];
    __shared__ int chain_s[BRIDGES_REC_K];
    const int g = blockIdx.x;
    beam_trace_load(a, g, par_s, val_s);
    __syncthreads();
    if (threadIdx.x == 0) {
        bool broken;
        beam_trace_walk(a, g, par_s, val_s, chain_s, broken);
        status[g] = broken ? 1 : 0;
    }
}

__global__ __launch_bounds__(BEAM_THREADS) void k_beam_trace_rows(BeamTraceArgs a, const int32_t* __restrict__ status,
                                                                  double* __restrict__ out, int32_t* __restrict__ offset) {
    __shared__ int par_s[BEAM_THREADS];
    __shared__ uint8_t val_s[BEAM_THREADS];
    __shared__ int chain_s[BRIDGES_REC_K];
    __shared__ double lin_s[BRIDGES_REC_K], stable_s[BRIDGES_REC_K], g_s[BRIDGES_REC_K];
    __shared__ int part_s[BEAM_THREADS / WAVE];
    __shared__ int len_s;
    const int g = blockIdx.x, G = gridDim.x, t = threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
    beam_trace_load(a, g, par_s, val_s);
    // the rows of the groups in front of this one (of all groups, for the last: the total)
    const int upto = g == G - 1 ? G : g;
    int mine = 0, own = 0;
    for (int j = t; j < upto; j += BEAM_THREADS) {
        const int ed = a.end_depth[j];
        const int n = (ed >= 0 && status[j] == 0) ? ed + 1 : 0;
        if (j < g) mine += n; else own = n;
    }
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) mine += __shfl_xor(mine, m);
    if (lane == 0) part_s[wv] = mine;
    __syncthreads();
    if (t == 0) {
        bool broken;
        len_s = beam_trace_walk(a, g, par_s, val_s, chain_s, broken);
    }
    __syncthreads();
    int off = 0;
    for (int k = 0; k < BEAM_THREADS / WAVE; ++k) off += part_s[k];
    const int L = len_s;
    if (t == 0) offset[g] = off;
    if (g == G - 1 && (G - 1) % BEAM_THREADS == t) offset[G] = off + own;       // (the lane that read the last group's count)
    if (L == 0) return;
    const int e0 = g * a.B;
    constexpr int RW = BRIDGES_REC_WIDTH;
    if (t < L) {
        const double* r = a.rec + ((size_t)t * a.E + e0 + chain_s[t]) * RW;
        lin_s[t] = r[BRIDGES_REC_LIN];
        stable_s[t] = r[BRIDGES_REC_STABLE_S];
    }
    __syncthreads();
    if (t < L) {                                            // the return of start t, by one lane, in the order of the fold
        const int h = a.n_step < L - t ? a.n_step : L - t;
        double acc = 0.0, disc = 1.0;
        for (int k = 0; k < h; ++k) {
            acc += disc * lin_s[t + k];
            disc *= a.gamma;
        }
        g_s[t] = acc;
    }
    __syncthreads();
    const int Wo = RW + a.n_tail + (a.n_step > 1 ? 1 : 0);
    const uint64_t* tail = reinterpret_cast<const uint64_t*>(a.tail) + (size_t)a.end_env[g] * a.n_tail;   // (end_env lies in the group)
    for (int s = wv; s < L; s += BEAM_THREADS / WAVE) {     // a wave per row, its lanes on consecutive doubles
        const int h = a.n_step < L - s ? a.n_step : L - s;
        const int last = s + h - 1;
        const uint64_t* src = reinterpret_cast<const uint64_t*>(a.rec + ((size_t)last * a.E + e0 + chain_s[last]) * RW);
        uint64_t* dst = reinterpret_cast<uint64_t*>(out + ((size_t)off + s) * Wo);
        for (int col = lane; col < Wo; col += WAVE) {
            uint64_t v;
            if (col < RW) {
                v = src[col];
                if (col == BRIDGES_REC_STABLE_S) v = (uint64_t)__double_as_longlong(stable_s[s]);
                if (col == BRIDGES_REC_TD) v = (uint64_t)__double_as_longlong(a.priority);
                if (col == BRIDGES_REC_LIN && h > 1) v = (uint64_t)__double_as_longlong(g_s[s]);
            } else if (col < RW + a.n_tail) {
                v = tail[col - RW];
            } else {
                v = (uint64_t)__double_as_longlong((double)h);
            }
            dst[col] = v;
        }
    }
}

}  // namespace bridges
