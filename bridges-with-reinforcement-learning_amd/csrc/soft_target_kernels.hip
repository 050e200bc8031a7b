// Expected-value TD targets under the Boltzmann policy (bridges_soft_expect; the rule stands in include/bridges_hip.h).
#include "bridges_device.h"

namespace bridges {

// ---------------------------------------------------------------------------------------------------------------
// For transition i with the rows lo .. hi - 1 of select_q / next_q / feat:
//   p_j = w_j / Z,  w_j = boltzmann_weight(select_q_j, m, T)  (k_boltzmann_select's weights, by its very function),
//   value[i] = sum_j p_j next_q_j,  feat_mean[i, c] = sum_j p_j feat[r_j, c],  entropy[i] = log Z - sum_j p_j x_j,
//   argmax_row[i] = the first eligible row that holds m.
// One 256-lane workgroup per (transition, tile of SOFT_TILE columns); a lane owns four consecutive columns of its tile.
//   phase A: the lanes stride the segment's select_q three times -- the maximum, then Z and the first maximum, then the p_j,
//            which go to LDS SOFT_CHUNK rows at a time together with the rows' offsets into feat (so no segment length is
//            assumed).  Wave results come off the DPP tree, the four waves' pass through LDS and are combined in wave order.
//            Every tile recomputes this: a segment's q is a few hundred bytes, and ranges may overlap, so weights kept in
//            memory would need a slot per (transition, row).  Tile 0 alone forms value, entropy and argmax_row.
//   phase B: the workgroup walks the chunk's rows ascending, SOFT_ROWS at a time: the loads of the rows that weigh anything
//            are issued first (16 B per lane where base, stride and dim allow it, else element by element), then
//            acc += p_j * (double)f in row order, product and sum rounded separately.  A row whose weight is exactly 0 is
//            neither loaded nor added.  The four float64 sums are rounded to float32 once and stored.
// No atomics, every output word written once, every sum in a fixed order: the same inputs give the same bits.
constexpr int SOFT_TILE = 1024;                          // columns per workgroup: 256 lanes x 4
constexpr int SOFT_CHUNK = 1024;                         // rows whose p_j and offsets LDS holds at a time (16 KiB)
constexpr int SOFT_ROWS = 4;                             // rows whose loads are in flight before the first use

// The four waves' values, combined in wave order behind one barrier; `slot` is a [4] array in LDS used for nothing else.
__device__ __forceinline__ double soft_block_sum(double wave_value, double* slot, int t) {
    if ((t & (WAVE - 1)) == 0) slot[t / WAVE] = wave_value;
    __syncthreads();
    return ((slot[0] + slot[1]) + slot[2]) + slot[3];
}

// One body for k_soft_expect and k_soft_expect_rel.  REL: the temperature of transition i is relative_temperature() of the spread
// of its rows of select_q (segment_spread of dqn_kernels.hip through the LDS wave-combine, three slots of its own), taken in phase
// A between pass 1 and the Z pass by every tile; tile 0 writes it to temp_out[i] (nothing eligible: no row is finite either, so
// temperature * spread_floor without a pass).
template <bool REL>
__device__ __forceinline__ void soft_expect_body(int n_trans, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                 const float* select_q, const float* next_q, float temperature, float spread_floor,
                                                 const float* __restrict__ feat, int64_t feat_row_stride,
                                                 const int64_t* __restrict__ feat_row, int dim, float* __restrict__ value,
                                                 float* __restrict__ feat_mean, float* __restrict__ entropy,
                                                 int32_t* __restrict__ argmax_row, double* __restrict__ temp_out) {
    constexpr int NONE = 0x7fffffff;
    __shared__ double s_spread[REL ? 3 : 1][4];          // (never referenced without REL: the compiler drops it)
    __shared__ double s_p[SOFT_CHUNK];
    __shared__ int64_t s_off[SOFT_CHUNK];
    __shared__ double s_m[4], s_z[4], s_v[4], s_e[4];
    __shared__ int s_fm[4];
    const int i = blockIdx.x, tile = blockIdx.y, t = threadIdx.x;
    if (i >= n_trans) return;                            // (uniform per workgroup: the grid is n_trans x tiles)
    const int lo = seg_lo[i], hi = seg_hi[i];
    double T = (double)temperature;
    const bool first_tile = tile == 0;

    // phase A, pass 1: the largest eligible q (-inf: nothing is eligible; that includes the empty segment)
    double mx = -(double)INFINITY;
    for (int j = lo + t; j < hi; j += 256) {
        const float v = select_q[j];
        if (v == v && (double)v > mx) mx = (double)v;
    }
    mx = wave_max_d(mx);
    if ((t & (WAVE - 1)) == 0) s_m[t / WAVE] = mx;
    __syncthreads();
    const double m = fmax(fmax(s_m[0], s_m[1]), fmax(s_m[2], s_m[3]));
    const bool any = m != -(double)INFINITY;             // uniform

    const int c0 = tile * SOFT_TILE + 4 * t;             // this lane's first column
    const int nc = dim - c0 < 4 ? dim - c0 : 4;          // how many of its four exist (<= 0: none)
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (REL) {
        double spread = 0.0;
        if (any) spread = segment_spread<256>(select_q, lo, hi, t, [&](double v, int k) { return soft_block_sum(v, s_spread[k], t); });
        T = relative_temperature(temperature, spread, spread_floor);
        if (first_tile && t == 0) temp_out[i] = T;
    }
    if (any) {
        // pass 2: Z and the first row that holds the maximum
        double z = 0.0;
        int fm = NONE;
        for (int j = lo + t; j < hi; j += 256) {
            const float v = select_q[j];
            if (fm == NONE && v == v && (double)v == m) fm = j;
            z += boltzmann_weight(v, m, T);
        }
        fm = wave_min_i(fm);
        if ((t & (WAVE - 1)) == 0) s_fm[t / WAVE] = fm;
        const double Z = soft_block_sum(wave_sum_d(z), s_z, t);          // (its barrier publishes s_fm too)
        // pass 3: p_j and the rows' offsets to LDS chunk by chunk, phase B behind each chunk
        const bool vec_in = ((((uintptr_t)feat) & 15) | (uintptr_t)(feat_row_stride & 3)) == 0 && nc == 4;
        double val = 0.0, ent = 0.0;
        for (int base = lo; base < hi; base += SOFT_CHUNK) {
            const int rows = hi - base < SOFT_CHUNK ? hi - base : SOFT_CHUNK;
            for (int k = t; k < rows; k += 256) {
                const int j = base + k;
                const float v = select_q[j];
                const double p = boltzmann_weight(v, m, T) / Z;
                int64_t off = 0;
                if (p != 0.0) {
                    if (dim > 0) off = (feat_row ? feat_row[j] : (int64_t)j) * feat_row_stride;
                    if (first_tile) {
                        val += p * (double)next_q[j];
                        if (m != (double)INFINITY) ent += p * (((double)v - m) / T);    // (m = +inf: x_j = 0 on its rows)
                    }
                }
                s_p[k] = p;
                s_off[k] = off;
            }
            __syncthreads();
            if (nc > 0) {
                const float* col = feat + c0;
                for (int k = 0; k < rows; k += SOFT_ROWS) {
                    double p[SOFT_ROWS];
                    float4 f[SOFT_ROWS];
#pragma unroll
                    for (int u = 0; u < SOFT_ROWS; ++u) {
                        p[u] = k + u < rows ? s_p[k + u] : 0.0;
                        f[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (p[u] != 0.0) {
                            const float* src = col + s_off[k + u];
                            if (vec_in) {
                                f[u] = *reinterpret_cast<const float4*>(src);
                            } else {
                                f[u].x = src[0];
                                if (nc > 1) f[u].y = src[1];
                                if (nc > 2) f[u].z = src[2];
                                if (nc > 3) f[u].w = src[3];
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < SOFT_ROWS; ++u) {
                        if (p[u] != 0.0) {
                            a0 += p[u] * (double)f[u].x; a1 += p[u] * (double)f[u].y;
                            a2 += p[u] * (double)f[u].z; a3 += p[u] * (double)f[u].w;
                        }
                    }
                }
            }
            __syncthreads();                             // the next chunk overwrites s_p / s_off
        }
        if (first_tile) {                                // uniform
            val = soft_block_sum(wave_sum_d(val), s_v, t);
            ent = soft_block_sum(wave_sum_d(ent), s_e, t);
            if (t == 0) {
                value[i] = (float)val;
                if (entropy) entropy[i] = (float)(log(Z) - ent);
                argmax_row[i] = min(min(s_fm[0], s_fm[1]), min(s_fm[2], s_fm[3]));
            }
        }
    } else if (first_tile && t == 0) {
        value[i] = -INFINITY;
        if (entropy) entropy[i] = 0.f;
        argmax_row[i] = NONE;
    }
    if (nc > 0) {
        float* dst = feat_mean + (int64_t)i * dim + c0;
        if (nc == 4 && (dim & 3) == 0 && (((uintptr_t)feat_mean) & 15) == 0) {
            *reinterpret_cast<float4*>(dst) = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
        } else {
            dst[0] = (float)a0;
            if (nc > 1) dst[1] = (float)a1;
            if (nc > 2) dst[2] = (float)a2;
            if (nc > 3) dst[3] = (float)a3;
        }
    }
}

__global__ __launch_bounds__(256) void k_soft_expect(int n_trans, const int32_t* __restrict__ seg_lo, const int32_t* __restrict__ seg_hi,
                                                     const float* select_q, const float* next_q, float temperature,
                                                     const float* __restrict__ feat, int64_t feat_row_stride,
                                                     const int64_t* __restrict__ feat_row, int dim, float* __restrict__ value,
                                                     float* __restrict__ feat_mean, float* __restrict__ entropy,
                                                     int32_t* __restrict__ argmax_row) {
    soft_expect_body<false>(n_trans, seg_lo, seg_hi, select_q, next_q, temperature, 0.f, feat, feat_row_stride, feat_row, dim, value,
                            feat_mean, entropy, argmax_row, nullptr);
}

__global__ __launch_bounds__(256) void k_soft_expect_rel(int n_trans, const int32_t* __restrict__ seg_lo,
                                                         const int32_t* __restrict__ seg_hi, const float* select_q, const float* next_q,
                                                         float temperature, float spread_floor, const float* __restrict__ feat,
                                                         int64_t feat_row_stride, const int64_t* __restrict__ feat_row, int dim,
                                                         float* __restrict__ value, float* __restrict__ feat_mean,
                                                         float* __restrict__ entropy, int32_t* __restrict__ argmax_row,
                                                         double* __restrict__ temp_out) {
    soft_expect_body<true>(n_trans, seg_lo, seg_hi, select_q, next_q, temperature, spread_floor, feat, feat_row_stride, feat_row, dim,
                           value, feat_mean, entropy, argmax_row, temp_out);
}

}  // namespace bridges
