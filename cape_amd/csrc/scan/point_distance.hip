// Mesh-to-scan distance for a batch of query sets (the mesh vertices) against a batch of point clouds (the scans), and its
// gradient: for every query the nearest point of its sample's cloud.  Per sample n and query j < Q, over the points
// i < count[n]:
//   d2(q, p) = |q - p|^2;   index[n, j] = argmin_i d2(q_j, p_i), the lowest index among equal fp32 values of the search
//   d2[n, j] = |q_j - p_index|^2 evaluated again in fp64 from the original fp32 coordinates, rounded once
// A point whose fp32 distance is not finite never wins; no such point (count 0, no finite point) or a query with a non-finite
// coordinate: index -1, d2 NaN, no gradient.
//
// Forward, two launches.  (1) search, fp32, in the difference form (q - p) on the raw coordinates: the difference of two nearby
// fp32 numbers is exact, so the rounding scales with the distance, not with the position -- no sample-local origin and no prep
// launch; the expanded form |q|^2 + |p|^2 - 2 q.p (and with it the matrix pipe) would cancel to a few per cent of a millimetre
// distance on a metre-sized body.  A workgroup of SB threads holds QB = QPT SB queries of one sample in registers and streams a
// range of the sample's points through LDS in tiles of PT float4; all lanes read the same point at the same time (one
// ds_read_b128 broadcast per QPT tests), and the best is kept with a strict `<` in increasing point order.  With few workgroups
// the points are split over `split` workgroups per query tile (a function of the sizes only); every part writes its
// (d2 bits, index) candidate.  (2) finish: the candidates are merged in increasing part order with the same strict `<` -- the
// result of the unsplit walk -- and the winner is evaluated in fp64.
//
// QPT = 2: the test is 9 VALU instructions (3 sub, mul, 2 fma, cmp, 2 cndmask), so one LDS read feeds 18 of them.  Measured
// on an MI355X at Q = 6890, M = 20000 (alternating sets, same bits from all three): 2 / 4 / 8 queries per thread take
// 469 / 462 / 482 us at N = 16 and 87 / 140 / 228 us at N = 1 -- more per thread saves nothing the VALU was waiting for, and
// fewer, larger workgroups fill the part worse when the grid is small.  The compiler reports 48 / 51 / 94 VGPRs: the register
// file does not decide.  DESIGN 7j has the figures.
//
// Backward, one or two launches, no atomics.  (1) per query: dq = 2 g (q - p_index) in fp64, rounded once, and -- when dp is
// wanted -- its negative as three doubles into the workspace.  (2) one thread per (sample, point): workgroups of points stream
// the sample's indices through LDS in query order and add the record where the index is theirs: fixed-order fp64 sums, the same
// inputs give the same bits.
#include "../common.h"

namespace {

constexpr int SB = 256;             // threads of a search workgroup
#ifndef CAPE_POINT_QPT
#define CAPE_POINT_QPT 2            // a build with another value (make EXTRA=-DCAPE_POINT_QPT=4) is for measuring it only
#endif
constexpr int QPT = CAPE_POINT_QPT; // queries per thread
constexpr int QB = SB * QPT;        // queries per workgroup
constexpr int PT = 512;             // points per LDS tile (8 KB of float4)
constexpr int SPLIT_MAX = 16;       // most workgroups that share one query tile's points
constexpr int TARGET_WG = 1024;     // split until about this many workgroups exist (four per compute unit: one wave per SIMD each)
constexpr int LB = 256;             // threads of the per-item kernels
constexpr int MAXB = 4096;
constexpr int GT = 2048;            // indices per LDS tile of the gather
constexpr int64_t REC = 3;          // doubles per query of the backward: -2 g (q - p)

struct Plan {
    int tiles;            // query tiles per sample
    int split;            // workgroups per query tile
    int tiles_per_part;   // point tiles each of them walks
};

// a function of the sizes only
inline Plan make_plan(int64_t N, int64_t Q, int64_t M) {
    Plan p;
    p.tiles = (int)((Q + QB - 1) / QB);
    const int64_t wg = N * p.tiles;
    const int64_t ptiles = (M + PT - 1) / PT;
    int64_t s = TARGET_WG / wg;
    if (s > SPLIT_MAX) s = SPLIT_MAX;
    if (s > ptiles) s = ptiles;
    if (s < 1) s = 1;
    p.tiles_per_part = (int)((ptiles + s - 1) / s);
    p.split = (int)((ptiles + p.tiles_per_part - 1) / p.tiles_per_part);
    return p;
}

// work items and indices are int32
inline bool sizes_ok(int64_t N, int64_t Q, int64_t M) {
    const int64_t lim = (int64_t)1 << 31;
    return N >= 1 && Q >= 1 && M >= 1 && N * Q < lim && N * M < lim;
}

inline int64_t fwd_bytes(int64_t N, int64_t Q, int64_t M) { return (int64_t)make_plan(N, Q, M).split * N * Q * 8; }
inline int64_t bwd_bytes(int64_t N, int64_t Q) { return N * Q * REC * 8; }

__device__ __forceinline__ int clamp_count(const int *count, long long n, int M) {
    if (!count) return M;
    const int c = count[n];
    return c < 0 ? 0 : (c > M ? M : c);
}

// ---- forward (1): the fp32 search ------------------------------------------------------------------------------------------------
// grid: N * split * tiles workgroups, the query tile fastest.  cand [split][N Q] (d2 bits, index), written for every query: a part
// whose range lies beyond count[n] writes (inf, -1).
__global__ __launch_bounds__(SB) void point_search_kernel(const float *q, int ldq, const float *pts, int ldp, const int *count,
                                                          int Q, int M, int tiles, int split, int tiles_per_part, long long NQ,
                                                          uint2 *cand) {
    __shared__ float4 tile[PT];
    const int t = blockIdx.x % tiles;
    const int part = (blockIdx.x / tiles) % split;
    const long long n = blockIdx.x / (tiles * split);
    const int cnt = clamp_count(count, n, M);
    const int j0 = t * QB;
    float qx[QPT], qy[QPT], qz[QPT], best[QPT];
    int bi[QPT];
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int j = j0 + k * SB + threadIdx.x;
        qx[k] = qy[k] = qz[k] = 0.0f;
        if (j < Q) {
            const float *s = q + (n * Q + j) * ldq;
            qx[k] = s[0];
            qy[k] = s[1];
            qz[k] = s[2];
        }
        best[k] = __builtin_inff();
        bi[k] = -1;
    }
    const long long i_begin = (long long)part * tiles_per_part * PT;       // a range of the M rows: the split never looks at count
    const long long i_stop = i_begin + (long long)tiles_per_part * PT;
    const int i_end = (int)(i_stop < cnt ? i_stop : cnt);                   // padding points are never read
    for (long long i0l = i_begin; i0l < i_end; i0l += PT) {                 // uniform over the workgroup
        const int i0 = (int)i0l;
        const int np = i_end - i0 < PT ? i_end - i0 : PT;
        __syncthreads();                                                    // the previous tile has been read by every wave
        for (int i = threadIdx.x; i < np; i += SB) {
            const float *s = pts + (n * M + i0 + i) * ldp;
            tile[i] = make_float4(s[0], s[1], s[2], 0.0f);
        }
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < np; ++i) {
            const float4 p = tile[i];
#pragma unroll
            for (int k = 0; k < QPT; ++k) {
                const float dx = qx[k] - p.x, dy = qy[k] - p.y, dz = qz[k] - p.z;
                const float d = __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx));
                if (d < best[k]) {                                          // strict: the lowest point among ties, never a NaN or an inf
                    best[k] = d;
                    bi[k] = i0 + i;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int j = j0 + k * SB + threadIdx.x;
        if (j < Q) cand[(long long)part * NQ + n * Q + j] = make_uint2(__float_as_uint(best[k]), (unsigned)bi[k]);
    }
}

// ---- forward (2): merge and the fp64 evaluation of the winner -------------------------------------------------------------------
__global__ __launch_bounds__(LB) void point_finish_kernel(const float *q, int ldq, const float *pts, int ldp, const uint2 *cand,
                                                          int split, int N, int Q, int M, int *index, float *d2) {
    const long long total = (long long)N * Q;
    for (long long idx = (long long)blockIdx.x * LB + threadIdx.x; idx < total; idx += (long long)gridDim.x * LB) {
        const long long n = idx / Q;
        int id = -1;
        float best = __builtin_inff();
        for (int s = 0; s < split; ++s) {                                   // parts hold increasing point ranges
            const uint2 c = cand[(long long)s * total + idx];
            const float d = __uint_as_float(c.x);
            if (d < best) {
                best = d;
                id = (int)c.y;
            }
        }
        float out = __builtin_nanf("");
        if (id >= 0 && id < M) {
            const float *a = q + idx * ldq, *b = pts + (n * M + id) * ldp;
            const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
            const double dd = dx * dx + dy * dy + dz * dz;
            if (isfinite(dd)) out = (float)dd;
            else id = -1;
        } else {
            id = -1;
        }
        index[idx] = id;
        d2[idx] = out;
    }
}

// ---- backward (1): per query -----------------------------------------------------------------------------------------------------
// rec NULL: dp is not wanted
__global__ __launch_bounds__(LB) void point_query_grad_kernel(const float *q, int ldq, const float *pts, int ldp, const int *count,
                                                              const int *index, const float *g, int N, int Q, int M, float *dq,
                                                              int lddq, double *rec) {
    const long long total = (long long)N * Q;
    for (long long idx = (long long)blockIdx.x * LB + threadIdx.x; idx < total; idx += (long long)gridDim.x * LB) {
        const long long n = idx / Q;
        const int id = index[idx];
        double rx = 0.0, ry = 0.0, rz = 0.0;
        if (id >= 0 && id < clamp_count(count, n, M)) {                     // -1: a query without a nearest point
            const float *a = q + idx * ldq, *b = pts + (n * M + id) * ldp;
            const double g2 = 2.0 * (double)g[idx];
            rx = g2 * ((double)a[0] - (double)b[0]);
            ry = g2 * ((double)a[1] - (double)b[1]);
            rz = g2 * ((double)a[2] - (double)b[2]);
        }
        float *o = dq + idx * lddq;
        o[0] = (float)rx;
        o[1] = (float)ry;
        o[2] = (float)rz;
        if (rec) {
            double *r = rec + idx * REC;
            r[0] = -rx, r[1] = -ry, r[2] = -rz;
        }
    }
}

// ---- backward (2): gather per point ----------------------------------------------------------------------------------------------
// grid: N * ptiles workgroups.  The indices are compared 16 at a time without a branch (four ds_read_b128 broadcasts in flight, a
// 16-bit match mask); the rare matches are then added in increasing query order.  One compare and branch per index instead
// leaves every LDS read waiting for the branch before it: measured at Q = 6890, M = 20000 the launch's share of a call fell from
// 373 to 57 us at N = 1 and from 414 to 183 us at N = 16.
__global__ __launch_bounds__(LB) void point_gather_kernel(const int *index, const double *rec, const int *count, int Q, int M,
                                                          int ptiles, float *dp, int lddp) {
    __shared__ __align__(16) int tile[GT];
    const long long n = blockIdx.x / ptiles;
    const int i = (blockIdx.x % ptiles) * LB + threadIdx.x;
    const bool mine = i < clamp_count(count, n, M);                         // padding rows match nothing and are written as zero
    const int *src = index + n * Q;
    const double *rs = rec + n * Q * REC;
    const int4 *t4 = (const int4 *)tile;
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int j0 = 0; j0 < Q; j0 += GT) {
        const int nq = Q - j0 < GT ? Q - j0 : GT;
        const int nq16 = (nq + 15) & ~15;                                   // at most GT, a multiple of 16
        __syncthreads();
        for (int j = threadIdx.x; j < nq16; j += LB) tile[j] = j < nq ? src[j0 + j] : -1;
        __syncthreads();
        for (int c = 0; c < nq16; c += 16) {
            unsigned mask = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int4 a = t4[c / 4 + u];
                mask |= ((unsigned)(a.x == i) | ((unsigned)(a.y == i) << 1) | ((unsigned)(a.z == i) << 2) | ((unsigned)(a.w == i) << 3))
                        << (4 * u);
            }
            if (!mine) mask = 0;
            while (mask) {                                                  // increasing query order
                const int b = __ffs((int)mask) - 1;
                mask &= mask - 1;
                const double *r = rs + (long long)(j0 + c + b) * REC;
                ax += r[0];
                ay += r[1];
                az += r[2];
            }
        }
    }
    if (i < M) {
        float *o = dp + (n * M + i) * lddp;
        o[0] = (float)ax;
        o[1] = (float)ay;
        o[2] = (float)az;
    }
}

}  // namespace

extern "C" int64_t cape_point_distance_workspace_bytes(int32_t N, int32_t Q, int32_t M) {
    if (!sizes_ok(N, Q, M)) return CAPE_EINVAL;
    const int64_t a = fwd_bytes(N, Q, M), b = bwd_bytes(N, Q);
    return a > b ? a : b;
}

extern "C" int cape_point_distance_plan(int32_t N, int32_t Q, int32_t M, int32_t *plan) {
    if (!plan || !sizes_ok(N, Q, M)) return CAPE_EINVAL;
    plan[0] = make_plan(N, Q, M).split;
    plan[1] = PT;
    plan[2] = QB;
    return CAPE_OK;
}

extern "C" int cape_point_nearest_fwd(const float *q, int32_t ldq, const float *points, int32_t ldp, const int32_t *count,
                                      int32_t N, int32_t Q, int32_t M, int32_t *index, float *d2, void *workspace,
                                      int64_t workspace_bytes, void *stream) {
    if (!q || !points || !index || !d2 || !workspace) return CAPE_EINVAL;
    if (!sizes_ok(N, Q, M) || ldq < 3 || ldp < 3) return CAPE_EINVAL;
    if (((uintptr_t)workspace & 15) != 0 || workspace_bytes < fwd_bytes(N, Q, M)) return CAPE_EINVAL;
    const Plan p = make_plan(N, Q, M);
    const long long groups = (long long)N * p.split * p.tiles;
    if (groups >= ((long long)1 << 31)) return CAPE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    uint2 *cand = (uint2 *)workspace;
    CAPE_LAUNCH(point_search_kernel, dim3((unsigned)groups), dim3(SB), 0, st, q, ldq, points, ldp, count, Q, M, p.tiles, p.split,
                p.tiles_per_part, (long long)N * Q, cand);
    CAPE_LAUNCH_CHECK();
    CAPE_LAUNCH(point_finish_kernel, dim3(cape_grid_blocks((long long)N * Q, LB, MAXB)), dim3(LB), 0, st, q, ldq, points, ldp,
                (const uint2 *)cand, p.split, N, Q, M, index, d2);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

extern "C" int cape_point_nearest_bwd(const float *q, int32_t ldq, const float *points, int32_t ldp, const int32_t *count,
                                      const int32_t *index, const float *g, int32_t N, int32_t Q, int32_t M, float *dq,
                                      int32_t lddq, float *dp, int32_t lddp, void *workspace, int64_t workspace_bytes,
                                      void *stream) {
    if (!q || !points || !index || !g || !dq || !workspace) return CAPE_EINVAL;
    if (!sizes_ok(N, Q, M) || ldq < 3 || ldp < 3 || lddq < 3 || (dp && lddp < 3)) return CAPE_EINVAL;
    if (((uintptr_t)workspace & 15) != 0 || workspace_bytes < bwd_bytes(N, Q)) return CAPE_EINVAL;
    const int ptiles = (M + LB - 1) / LB;
    const long long groups = (long long)N * ptiles;
    if (groups >= ((long long)1 << 31)) return CAPE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    double *rec = dp ? (double *)workspace : nullptr;
    CAPE_LAUNCH(point_query_grad_kernel, dim3(cape_grid_blocks((long long)N * Q, LB, MAXB)), dim3(LB), 0, st, q, ldq, points, ldp,
                count, index, g, N, Q, M, dq, lddq, rec);
    CAPE_LAUNCH_CHECK();
    if (dp) {
        CAPE_LAUNCH(point_gather_kernel, dim3((unsigned)groups), dim3(LB), 0, st, index, (const double *)rec, count, Q, M, ptiles,
                    dp, lddp);
        CAPE_LAUNCH_CHECK();
    }
    return CAPE_OK;
}
