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
// distance on a metre-sized body.  The skeleton is nearest.h's: QB = QPT SB queries per workgroup, points through LDS in tiles
// of PT float4 (one ds_read_b128 broadcast per QPT tests).  (2) finish: nearest.h's merge, the winner evaluated in fp64.
//
// QPT = 2: the test is 9 VALU instructions (3 sub, mul, 2 fma, cmp, 2 cndmask), so one LDS read feeds 18 of them.  Measured
// on an MI355X at Q = 6890, M = 20000 (alternating sets, same bits from all three): 2 / 4 / 8 queries per thread take
// 469 / 462 / 482 us at N = 16 and 87 / 140 / 228 us at N = 1 -- more per thread saves nothing the VALU was waiting for, and
// fewer, larger workgroups fill the part worse when the grid is small.  The compiler reports 48 / 51 / 94 VGPRs: the register
// file does not decide.  DESIGN 7j has the figures.
//
// The normal-compatible forward (cape_point_nearest_compat_fwd) stages a second float4 per point, its normal, and
// leaves the points whose normal disagrees with the query's out of the minimum; finish and backward are shared.
//
// Backward, one or two launches, no atomics.  (1) per query: dq = 2 g (q - p_index) in fp64, rounded once, and -- when dp is
// wanted -- its negative as three doubles into the workspace.  (2) one thread per (sample, point): workgroups of points stream
// the sample's indices through LDS in query order and add the record where the index is theirs: fixed-order fp64 sums, the same
// inputs give the same bits.
#include "nearest.h"

namespace {

using namespace nearest;

#ifndef CAPE_POINT_QPT
#define CAPE_POINT_QPT 2            // a build with another value (make EXTRA=-DCAPE_POINT_QPT=4) is for measuring it only
#endif
constexpr int QPT = CAPE_POINT_QPT; // queries per thread
constexpr int QB = SB * QPT;        // queries per workgroup
constexpr int PT = 512;             // points per LDS tile (8 KB of float4)
constexpr int TARGET_WG = 1024;     // split until about this many workgroups exist (four per compute unit: one wave per SIMD each)
constexpr int GT = 2048;            // indices per LDS tile of the gather
constexpr int64_t REC = 3;          // doubles per query of the backward: -2 g (q - p)

inline Plan point_plan(int64_t N, int64_t Q, int64_t M) { return make_plan(N, Q, QB, M, PT, TARGET_WG, SPLIT_MAX); }

// work items and indices are int32
inline bool sizes_ok(int64_t N, int64_t Q, int64_t M) {
    const int64_t lim = (int64_t)1 << 31;
    return N >= 1 && Q >= 1 && M >= 1 && N * Q < lim && N * M < lim;
}

inline int64_t fwd_bytes(int64_t N, int64_t Q, int64_t M) { return cand_bytes(N, Q, point_plan(N, Q, M)); }
inline int64_t bwd_bytes(int64_t N, int64_t Q) { return N * Q * REC * 8; }

// ---- forward (1): the fp32 search ------------------------------------------------------------------------------------------------
// raw queries against raw points in the difference form; every query gets a candidate, (inf, -1) from a part beyond count[n]
struct PointSearch {
    static constexpr int QPT = ::QPT, TILE = PT, REC = 1, UNROLL = 4;
    using Row = long long;                                                  // M + PT may pass 2^31
    struct Args {
        const float *q;
        int ldq;
        const float *pts;
        int ldp, Q, M;
    };
    static __device__ __forceinline__ void load_query(const Args &a, long long n, int j, float &qx, float &qy, float &qz) {
        const float *s = a.q + (n * a.Q + j) * a.ldq;
        qx = s[0];
        qy = s[1];
        qz = s[2];
    }
    static __device__ __forceinline__ void stage(const Args &a, float4 *tile, long long n, int i0, int np) {
        for (int i = threadIdx.x; i < np; i += SB) {
            const float *s = a.pts + (n * a.M + i0 + i) * a.ldp;
            tile[i] = make_float4(s[0], s[1], s[2], 0.0f);
        }
    }
    static __device__ __forceinline__ float d2(float qx, float qy, float qz, const float4 (&p)[1]) {
        const float dx = qx - p[0].x, dy = qy - p[0].y, dz = qz - p[0].z;
        return __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx));               // never a NaN or an inf wins the strict `<`
    }
};

__global__ __launch_bounds__(SB) void point_search_kernel(const float *q, int ldq, const float *pts, int ldp, const int *count,
                                                          int Q, int M, int tiles, int split, int tiles_per_part, long long NQ,
                                                          uint2 *cand) {
    __shared__ float4 tile[PT];
    const long long n = blockIdx.x / (tiles * split);
    const PointSearch::Args a = {q, ldq, pts, ldp, Q, M};
    nearest_search<PointSearch>(a, tile, n, Q, Q, clamp_count(count, n, M), tiles, split, tiles_per_part, NQ, cand);
}

// The normal-compatible search: both sides carry a normal, and a point takes part in the minimum only if
// c = fma(qn.z, pn.z, fma(qn.y, pn.y, qn.x pn.x)) >= cos_min in fp32 -- `d = compatible ? d : inf` in front of the skeleton's
// strict `<`.  The staged point is two float4: the position, and the normal in what is padding in the plain tile (a second LDS
// broadcast per test).  Normals are used as given; one with a component that is not finite is held as NaN on either side and is
// compatible with nothing.
struct PointSearchCompat {
    static constexpr int QPT = ::QPT, TILE = PT, REC = 2, UNROLL = 4;
    using Row = long long;
    struct Extra {
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    };
    struct Args {
        PointSearch::Args s;
        const float *qn;
        int ldqn;
        const float *pn;
        int ldpn;
        float cos_min;
    };
    static __device__ __forceinline__ void load_query(const Args &a, long long n, int j, float &qx, float &qy, float &qz, Extra &e) {
        PointSearch::load_query(a.s, n, j, qx, qy, qz);
        const float *s = a.qn + (n * a.s.Q + j) * a.ldqn;
        const bool ok = isfinite(s[0]) && isfinite(s[1]) && isfinite(s[2]);
        e.nx = ok ? s[0] : __builtin_nanf("");
        e.ny = s[1];
        e.nz = s[2];
    }
    static __device__ __forceinline__ void stage(const Args &a, float4 *tile, long long n, int i0, int np) {
        for (int i = threadIdx.x; i < np; i += SB) {
            const float *s = a.s.pts + (n * a.s.M + i0 + i) * a.s.ldp, *m = a.pn + (n * a.s.M + i0 + i) * a.ldpn;
            const bool ok = isfinite(m[0]) && isfinite(m[1]) && isfinite(m[2]);
            tile[2 * i] = make_float4(s[0], s[1], s[2], 0.0f);
            tile[2 * i + 1] = make_float4(ok ? m[0] : __builtin_nanf(""), m[1], m[2], 0.0f);
        }
    }
    static __device__ __forceinline__ float d2(const Args &a, float qx, float qy, float qz, const Extra &e, const float4 (&p)[2]) {
        const float dx = qx - p[0].x, dy = qy - p[0].y, dz = qz - p[0].z;
        const float d = __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx));
        const float c = __fmaf_rn(e.nz, p[1].z, __fmaf_rn(e.ny, p[1].y, e.nx * p[1].x));
        return c >= a.cos_min ? d : __builtin_inff();                       // a NaN c is compatible with nothing
    }
};

__global__ __launch_bounds__(SB) void point_search_compat_kernel(const float *q, int ldq, const float *pts, int ldp, const float *qn,
                                                                 int ldqn, const float *pn, int ldpn, float cos_min,
                                                                 const int *count, int Q, int M, int tiles, int split,
                                                                 int tiles_per_part, long long NQ, uint2 *cand) {
    __shared__ float4 tile[PT * 2];
    const long long n = blockIdx.x / (tiles * split);
    const PointSearchCompat::Args a = {{q, ldq, pts, ldp, Q, M}, qn, ldqn, pn, ldpn, cos_min};
    nearest_search<PointSearchCompat>(a, tile, n, Q, Q, clamp_count(count, n, M), tiles, split, tiles_per_part, NQ, cand);
}

// ---- forward (2): the fp64 evaluation of the winner; none, or one whose fp64 distance is not finite: index -1, d2 NaN -----------
struct PointFinish {
    struct Args {
        const float *q;
        int ldq;
        const float *pts;
        int ldp, M;
        int *index;
        float *d2;
    };
    static __device__ __forceinline__ void write(const Args &a, long long n, long long idx, bool, int id) {
        float out = __builtin_nanf("");
        if (id >= 0 && id < a.M) {
            const float *u = a.q + idx * a.ldq, *v = a.pts + (n * a.M + id) * a.ldp;
            const double dx = (double)u[0] - (double)v[0], dy = (double)u[1] - (double)v[1], dz = (double)u[2] - (double)v[2];
            const double dd = dx * dx + dy * dy + dz * dz;
            if (isfinite(dd)) out = (float)dd;
            else id = -1;
        } else {
            id = -1;
        }
        a.index[idx] = id;
        a.d2[idx] = out;
    }
};

__global__ __launch_bounds__(LB) void point_finish_kernel(const float *q, int ldq, const float *pts, int ldp, const uint2 *cand,
                                                          int split, int N, int Q, int M, int *index, float *d2) {
    const PointFinish::Args a = {q, ldq, pts, ldp, M, index, d2};
    nearest_finish<PointFinish>(a, nullptr, cand, split, N, Q);
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
    plan[0] = point_plan(N, Q, M).split;
    plan[1] = PT;
    plan[2] = QB;
    return CAPE_OK;
}

extern "C" int cape_point_nearest_fwd(const float *q, int32_t ldq, const float *points, int32_t ldp, const int32_t *count,
                                      int32_t N, int32_t Q, int32_t M, int32_t *index, float *d2, void *workspace,
                                      int64_t workspace_bytes, void *stream) {
    if (!q || !points || !index || !d2 || !workspace) return CAPE_EINVAL;
    if (!sizes_ok(N, Q, M) || ldq < 3 || ldp < 3) return CAPE_EINVAL;
    const Plan p = point_plan(N, Q, M);
    const long long groups = search_groups(N, p);
    if (!launch_ok(workspace, workspace_bytes, fwd_bytes(N, Q, M), groups)) return CAPE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    uint2 *cand = (uint2 *)workspace;
    return forward(
        groups, (long long)N * Q,
        [&](dim3 grid, dim3 block) {
            CAPE_LAUNCH(point_search_kernel, grid, block, 0, st, q, ldq, points, ldp, count, Q, M, p.tiles, p.split,
                        p.tiles_per_part, (long long)N * Q, cand);
        },
        [&](dim3 grid, dim3 block) {
            CAPE_LAUNCH(point_finish_kernel, grid, block, 0, st, q, ldq, points, ldp, (const uint2 *)cand, p.split, N, Q, M, index,
                        d2);
        });
}

// the workspace is the plain entry's: cape_point_distance_workspace_bytes
extern "C" int cape_point_nearest_compat_fwd(const float *q, int32_t ldq, const float *points, int32_t ldp,
                                             const float *query_normals, int32_t ldqn, const float *point_normals, int32_t ldpn,
                                             float cos_min, const int32_t *count, int32_t N, int32_t Q, int32_t M, int32_t *index,
                                             float *d2, void *workspace, int64_t workspace_bytes, void *stream) {
    if (!q || !points || !query_normals || !point_normals || !index || !d2 || !workspace) return CAPE_EINVAL;
    if (!sizes_ok(N, Q, M) || ldq < 3 || ldp < 3 || ldqn < 3 || ldpn < 3 || cos_min != cos_min) return CAPE_EINVAL;
    const Plan p = point_plan(N, Q, M);
    const long long groups = search_groups(N, p);
    if (!launch_ok(workspace, workspace_bytes, fwd_bytes(N, Q, M), groups)) return CAPE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    uint2 *cand = (uint2 *)workspace;
    return forward(
        groups, (long long)N * Q,
        [&](dim3 grid, dim3 block) {
            CAPE_LAUNCH(point_search_compat_kernel, grid, block, 0, st, q, ldq, points, ldp, query_normals, ldqn, point_normals,
                        ldpn, cos_min, count, Q, M, p.tiles, p.split, p.tiles_per_part, (long long)N * Q, cand);
        },
        [&](dim3 grid, dim3 block) {
            CAPE_LAUNCH(point_finish_kernel, grid, block, 0, st, q, ldq, points, ldp, (const uint2 *)cand, p.split, N, Q, M, index,
                        d2);
        });
}

extern "C" int cape_point_nearest_bwd(const float *q, int32_t ldq, const float *points, int32_t ldp, const int32_t *count,
                                      const int32_t *index, const float *g, int32_t N, int32_t Q, int32_t M, float *dq,
                                      int32_t lddq, float *dp, int32_t lddp, void *workspace, int64_t workspace_bytes,
                                      void *stream) {
    if (!q || !points || !index || !g || !dq || !workspace) return CAPE_EINVAL;
    if (!sizes_ok(N, Q, M) || ldq < 3 || ldp < 3 || lddq < 3 || (dp && lddp < 3)) return CAPE_EINVAL;
    const int ptiles = (M + LB - 1) / LB;
    const long long groups = (long long)N * ptiles;
    if (!launch_ok(workspace, workspace_bytes, bwd_bytes(N, Q), groups)) return CAPE_EINVAL;
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
