// The exact nearest search that scan_distance.hip (points against faces) and point_distance.hip (vertices against points) share:
// per sample, every QUERY against every TARGET in fp32, the winner evaluated again in fp64.
// search: a workgroup of SB threads holds QPT SB queries of one sample in registers and streams a range of the sample's targets
// through LDS in tiles of TILE records; all lanes read the same record at the same time (an LDS broadcast) and the best is kept
// with a strict `<` in increasing target order.  With few workgroups the targets are split over `split` workgroups per query tile
// (make_plan: a function of the sizes only); every part writes one (d2 bits, id) candidate per query into cand [split][N queries].
// finish: the candidates are merged in increasing part order with the same strict `<` -- the result of the unsplit walk -- and the
// policy evaluates the winner in fp64 and writes its outputs.
// A direction is a policy: a struct of constants and static __device__ __forceinline__ members, no state (a by-reference lambda is
// not always inlined, and its closure then lives in scratch).
//   search policy   QPT, TILE, REC (float4 per target record), UNROLL (of the walk over a tile; 0: the compiler's choice),
//                   Row (the integer that walks the targets tile by tile: int only where targets + TILE fits one),
//                   struct Args (what the members read; built by the kernel from its own arguments),
//                   load_query(a, n, i, x, y, z), stage(a, tile, n, t0, nt), d2(x, y, z, r) -> fp32 squared distance
//   finish policy   struct Args, write(a, n, idx, valid, id): the outputs of query idx of sample n -- `valid` false: a padding row
//   query extras    a search policy may name a struct Extra (default-constructible): per-query registers beyond the position,
//                   such as a normal.  Its members then read load_query(a, n, i, x, y, z, extra) and d2(a, x, y, z, extra, r);
//                   a policy without one is called as above and compiles to what it compiled to before the extras existed.
// Which side `count` limits is two numbers per sample: the valid queries and the valid targets.  Rows beyond either are never read.
#pragma once
#include <type_traits>

#include "../common.h"

namespace nearest {

constexpr int SB = 256;             // threads of a search workgroup
constexpr int SPLIT_MAX = 16;       // most workgroups that share one query tile's targets
constexpr int LB = 256;             // threads of the per-item kernels
constexpr int MAXB = 4096;

struct Plan {
    int tiles;            // query tiles per sample
    int split;            // workgroups per query tile
    int tiles_per_part;   // target tiles each of them walks
};

// a function of the sizes only: split until about target_wg workgroups exist
inline Plan make_plan(int64_t N, int64_t queries, int queries_per_wg, int64_t targets, int targets_per_tile, int target_wg,
                      int split_max) {
    Plan p;
    p.tiles = (int)((queries + queries_per_wg - 1) / queries_per_wg);
    const int64_t wg = N * p.tiles;
    const int64_t ttiles = (targets + targets_per_tile - 1) / targets_per_tile;
    int64_t s = target_wg / wg;
    if (s > split_max) s = split_max;
    if (s > ttiles) s = ttiles;
    if (s < 1) s = 1;
    p.tiles_per_part = (int)((ttiles + s - 1) / s);
    p.split = (int)((ttiles + p.tiles_per_part - 1) / p.tiles_per_part);
    return p;
}

inline long long search_groups(int64_t N, const Plan &p) { return (long long)N * p.split * p.tiles; }
inline int64_t cand_bytes(int64_t N, int64_t queries, const Plan &p) { return (int64_t)p.split * N * queries * 8; }

// before an entry's first launch: a 16-byte aligned workspace of `need` bytes and a grid that fits int32
inline bool launch_ok(const void *workspace, int64_t workspace_bytes, int64_t need, long long groups) {
    return ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need && groups < ((long long)1 << 31);
}

// the forward's launches: search(grid, block), then finish(grid, block) over N * queries items
template <class Search, class Finish>
inline int forward(long long groups, long long items, Search search, Finish finish) {
    search(dim3((unsigned)groups), dim3(SB));
    CAPE_LAUNCH_CHECK();
    finish(dim3(cape_grid_blocks(items, LB, MAXB)), dim3(LB));
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

__device__ __forceinline__ int clamp_count(const int *count, long long n, int M) {
    if (!count) return M;
    const int c = count[n];
    return c < 0 ? 0 : (c > M ? M : c);
}

struct NoExtra {};
template <class P, class = void>
struct query_extra {
    using type = NoExtra;
    static constexpr bool present = false;
};
template <class P>
struct query_extra<P, std::void_t<typename P::Extra>> {
    using type = typename P::Extra;
    static constexpr bool present = true;
};

template <class P>
__device__ __forceinline__ void test_target(const typename P::Args &a, const float4 *tile, int j, int id, const float (&qx)[P::QPT],
                                            const float (&qy)[P::QPT], const float (&qz)[P::QPT],
                                            const typename query_extra<P>::type (&qe)[P::QPT], float (&best)[P::QPT],
                                            int (&bid)[P::QPT]) {
    float4 r[P::REC];
#pragma unroll
    for (int c = 0; c < P::REC; ++c) r[c] = tile[P::REC * j + c];
#pragma unroll
    for (int k = 0; k < P::QPT; ++k) {
        float d;
        if constexpr (query_extra<P>::present) d = P::d2(a, qx[k], qy[k], qz[k], qe[k], r);
        else d = P::d2(qx[k], qy[k], qz[k], r);
        if (d < best[k]) {                                                  // strict: the lowest id among ties, never a NaN
            best[k] = d;
            bid[k] = id;
        }
    }
}

// grid: N * split * tiles workgroups, the query tile fastest; n = blockIdx.x / (tiles * split).  `queries` rows per sample, of which
// the first `valid_queries` are searched and get a candidate; the targets below `valid_targets` are walked, and a part whose range
// lies beyond them writes (inf, -1).  tile: TILE * REC float4 of LDS.
template <class P>
__device__ __forceinline__ void nearest_search(const typename P::Args &a, float4 *tile, long long n, int queries, int valid_queries,
                                               int valid_targets, int tiles, int split, int tiles_per_part, long long NQ,
                                               uint2 *cand) {
    constexpr int QB = SB * P::QPT;
    const int t = blockIdx.x % tiles;
    const int part = (blockIdx.x / tiles) % split;
    const int i0 = t * QB;
    if (i0 >= valid_queries) return;                                        // the whole workgroup: no barrier is left waiting
    float qx[P::QPT], qy[P::QPT], qz[P::QPT], best[P::QPT];
    int bid[P::QPT];
    typename query_extra<P>::type qe[P::QPT];
#pragma unroll
    for (int k = 0; k < P::QPT; ++k) {
        const int i = i0 + k * SB + threadIdx.x;
        qx[k] = qy[k] = qz[k] = 0.0f;
        if (i < valid_queries) {
            if constexpr (query_extra<P>::present) P::load_query(a, n, i, qx[k], qy[k], qz[k], qe[k]);
            else P::load_query(a, n, i, qx[k], qy[k], qz[k]);
        }
        best[k] = __builtin_inff();
        bid[k] = -1;
    }
    using Row = typename P::Row;
    const Row t_begin = (Row)part * tiles_per_part * P::TILE;               // a range of the rows: the split never looks at count
    const Row t_stop = t_begin + (Row)tiles_per_part * P::TILE;
    const int t_end = (int)(t_stop < valid_targets ? t_stop : valid_targets);
    for (Row row = t_begin; row < t_end; row += P::TILE) {                  // uniform over the workgroup
        const int t0 = (int)row;
        const int nt = t_end - t0 < P::TILE ? t_end - t0 : P::TILE;
        __syncthreads();                                                    // the previous tile has been read by every wave
        P::stage(a, tile, n, t0, nt);
        __syncthreads();
        if constexpr (P::UNROLL > 0) {
#pragma unroll P::UNROLL
            for (int j = 0; j < nt; ++j) test_target<P>(a, tile, j, t0 + j, qx, qy, qz, qe, best, bid);
        } else {
            for (int j = 0; j < nt; ++j) test_target<P>(a, tile, j, t0 + j, qx, qy, qz, qe, best, bid);
        }
    }
#pragma unroll
    for (int k = 0; k < P::QPT; ++k) {
        const int i = i0 + k * SB + threadIdx.x;
        if (i < valid_queries) cand[(long long)part * NQ + n * queries + i] = make_uint2(__float_as_uint(best[k]), (unsigned)bid[k]);
    }
}

// the id of the unsplit walk's winner, -1 without one: parts hold increasing target ranges
__device__ __forceinline__ int merge_parts(const uint2 *cand, int split, long long total, long long idx) {
    int id = -1;
    float best = __builtin_inff();
    for (int s = 0; s < split; ++s) {
        const uint2 c = cand[(long long)s * total + idx];
        const float d = __uint_as_float(c.x);
        if (d < best) {
            best = d;
            id = (int)c.y;
        }
    }
    return id;
}

// one thread per (sample, query); count: what limits the valid queries of a sample, NULL: every row is one
template <class P>
__device__ __forceinline__ void nearest_finish(const typename P::Args &a, const int *count, const uint2 *cand, int split, int N,
                                               int queries) {
    const long long total = (long long)N * queries;
    for (long long idx = (long long)blockIdx.x * LB + threadIdx.x; idx < total; idx += (long long)gridDim.x * LB) {
        const int i = (int)(idx % queries);
        const long long n = idx / queries;
        const bool valid = i < clamp_count(count, n, queries);
        P::write(a, n, idx, valid, valid ? merge_parts(cand, split, total, idx) : -1);
    }
}

}  // namespace nearest
