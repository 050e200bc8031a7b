// bridges_env_fork: env e continues from the state of env src[e] (include/bridges_hip.h has the contract).
//
// A fork is a row gather over the caller-owned per-env state arrays.  The arrays are listed ONCE, in fork_table() below; the
// copy itself knows nothing about them.  Two launches of one kernel body: k_fork_rows<true> gathers row src[e] of every array
// into row e of the caller's scratch, k_fork_rows<false> writes scratch row e back to row e of the array.  No launch both reads
// and writes a state array, so a swap (src[e] = e ^ 1), a chain (src[e] = e + 1) or a broadcast is exact; no atomics, every
// byte written once: the same bits on every call.
//
// The copy is bandwidth-bound (the tableau rows lp_ws / lp_snap are 240 KiB / 120 KiB per env, everything else together about
// 10 KiB): plain vector loads and stores, 16 bytes per lane wherever an array's base and row size allow it, else the widest
// power of two that divides both.  A workgroup of 256 lanes moves one piece of at most FORK_PIECE bytes: for a long row a
// piece of one env's row (four 16-byte loads per lane in flight before the first store), for a short row the rows of several
// consecutive envs.  Whole rows are copied, the dead part of a tableau row included: the destination is then the source's
// row on every byte, whatever a later kernel reads of it.
#include "bridges_device.h"

namespace bridges {

#define FORK_MAX_ARRAYS 32
#define FORK_THREADS 256
#define FORK_PIECE 16384            // bytes per workgroup: 256 lanes x 16 B x 4 loads in flight

struct ForkArray {
    char* base;                     // row e of the array = base + e * row_bytes
    int64_t row_bytes;
    int64_t scratch_off;            // byte offset of the array's [E, row_bytes] image in the scratch (a multiple of 16)
    int32_t unit;                   // bytes per lane access: 16, 8, 4, 2 or 1 (divides base, row_bytes and scratch_off)
    int32_t rows_per_block;         // envs one workgroup handles (1 when a row is cut into pieces)
    int32_t pieces_per_row;         // workgroups per row (1 when a workgroup handles several rows)
    int32_t block0;                 // first workgroup of the array in the flattened grid
};

struct ForkTable {
    ForkArray a[FORK_MAX_ARRAYS];
    int32_t n, E;
    int64_t scratch_bytes;
    int32_t n_blocks;
};

template <typename U>
__device__ __forceinline__ void fork_copy_units(const char* __restrict__ from, char* __restrict__ to, int64_t n_units, int t) {
    const U* s = reinterpret_cast<const U*>(from);
    U* d = reinterpret_cast<U*>(to);
    int64_t i = t;
    for (; i + 3 * FORK_THREADS < n_units; i += 4 * FORK_THREADS) {        // all four loads first, then the stores
        const U v0 = s[i], v1 = s[i + FORK_THREADS], v2 = s[i + 2 * FORK_THREADS], v3 = s[i + 3 * FORK_THREADS];
        d[i] = v0; d[i + FORK_THREADS] = v1; d[i + 2 * FORK_THREADS] = v2; d[i + 3 * FORK_THREADS] = v3;
    }
    for (; i < n_units; i += FORK_THREADS) d[i] = s[i];
}

__device__ __forceinline__ void fork_copy(const char* from, char* to, int64_t bytes, int unit, int t) {
    switch (unit) {
        case 16: fork_copy_units<uint4>(from, to, bytes / 16, t); break;
        case 8: fork_copy_units<uint2>(from, to, bytes / 8, t); break;
        case 4: fork_copy_units<uint32_t>(from, to, bytes / 4, t); break;
        case 2: fork_copy_units<uint16_t>(from, to, bytes / 2, t); break;
        default: fork_copy_units<uint8_t>(from, to, bytes, t); break;
    }
}

// The env whose row env e takes: src[e], or e itself when src[e] lies outside [0, E).
__device__ __forceinline__ int fork_source(const int32_t* __restrict__ src, int e, int E) {
    const int s = src[e];
    return (s >= 0 && s < E) ? s : e;
}

// GATHER: scratch row e <- array row src[e].  !GATHER: array row e <- scratch row e (src is not read).
template <bool GATHER>
__global__ __launch_bounds__(FORK_THREADS) void k_fork_rows(ForkTable T, const int32_t* __restrict__ src, char* __restrict__ scratch) {
    const int t = threadIdx.x;
    const int blk = blockIdx.x;
    if (blk >= T.n_blocks) return;
    int ai = 0;                                             // the array this workgroup belongs to (uniform: scalar loop)
    while (ai + 1 < T.n && blk >= T.a[ai + 1].block0) ++ai;
    const ForkArray A = T.a[ai];
    const int local = blk - A.block0;
    if (A.pieces_per_row > 1 || A.rows_per_block == 1) {    // one piece of one env's row
        const int e = local / A.pieces_per_row, piece = local % A.pieces_per_row;
        if (e >= T.E) return;
        const int64_t off = (int64_t)piece * FORK_PIECE;
        int64_t len = A.row_bytes - off;
        if (len > FORK_PIECE) len = FORK_PIECE;
        if (len <= 0) return;
        char* in_scratch = scratch + A.scratch_off + (int64_t)e * A.row_bytes + off;
        if (GATHER) fork_copy(A.base + (int64_t)fork_source(src, e, T.E) * A.row_bytes + off, in_scratch, len, A.unit, t);
        else fork_copy(in_scratch, A.base + (int64_t)e * A.row_bytes + off, len, A.unit, t);
        return;
    }
    // several short rows: unit u of the workgroup's envs e0 .. e0 + rows - 1
    const int e0 = local * A.rows_per_block;
    int rows = T.E - e0;
    if (rows > A.rows_per_block) rows = A.rows_per_block;
    if (rows <= 0) return;
    if (!GATHER) {                                          // contiguous on both sides
        fork_copy(scratch + A.scratch_off + (int64_t)e0 * A.row_bytes, A.base + (int64_t)e0 * A.row_bytes, (int64_t)rows * A.row_bytes,
                  A.unit, t);
        return;
    }
    const int upr = (int)(A.row_bytes / A.unit);            // units per row
    for (int u = t; u < rows * upr; u += FORK_THREADS) {
        const int r = u / upr, col = u - r * upr;
        const int e = e0 + r;
        const char* from = A.base + (int64_t)fork_source(src, e, T.E) * A.row_bytes + (int64_t)col * A.unit;
        char* to = scratch + A.scratch_off + (int64_t)e * A.row_bytes + (int64_t)col * A.unit;
        switch (A.unit) {
            case 16: *reinterpret_cast<uint4*>(to) = *reinterpret_cast<const uint4*>(from); break;
            case 8: *reinterpret_cast<uint2*>(to) = *reinterpret_cast<const uint2*>(from); break;
            case 4: *reinterpret_cast<uint32_t*>(to) = *reinterpret_cast<const uint32_t*>(from); break;
            case 2: *reinterpret_cast<uint16_t*>(to) = *reinterpret_cast<const uint16_t*>(from); break;
            default: *to = *from; break;
        }
    }
}

}  // namespace bridges
