// Per-vertex Euclidean error of the evaluation (the reference's demos.py:68-78) and its statistics, on the device.
//   d[s, j] = sqrt( sum_c ((pred[s, idx[j], c] - gt[s, idx[j], c]) * std[idx[j], c])^2 )      (the mean cancels: not an operand)
// cape_vertex_error writes a batch's rows of dist [S, Vc]; cape_error_stats reduces the finished buffer:
//   mean / population variance (fp64, two passes: the mean first, then sum (d - mean)^2), per-sample and per-vertex means,
//   the count of non-finite values, and up to 8 exact order statistics by radix select on the fp32 bit patterns (d >= +0, so
//   the patterns order as unsigned integers): three digit passes of 11 / 11 / 10 bits.
// No kernel hands data to another workgroup of the same launch: every reduction ends in a launch of its own, every sum has
// a fixed order, the grids depend on the sizes only.  The one thing that crosses workgroups inside a launch is the digit
// histogram: integer device-scope adds, whose sum does not depend on the order; the next launch reads it.
#include <cmath>

#include "../common.h"

namespace {

constexpr int LB = 256;
constexpr int MAXB = 1024;                  // blocks of the grid-stride launches (and variance partials)
constexpr int MAXR = 8;                     // order statistics per call
constexpr int NBINS = 2048;                 // 11-bit digits (the last pass uses 1024 of them)
constexpr int HIST_ITEMS = 16384;           // elements per histogram block at least: one flush of R * NBINS bins per block
constexpr int HIST_MAXB = 512;
constexpr int PV_COLS = 16, PV_ROWS = 64;   // per-vertex block: 16 columns (64-byte row segments) x 64 row lanes

// device state of the radix select (uint32 words, at the start of the workspace)
constexpr int ST_PREFIX = 0, ST_REMAIN = MAXR, ST_GROUP = 2 * MAXR, ST_WORDS = 64;

struct Ranks {
    uint32_t r[MAXR];
};

__device__ __forceinline__ bool nonfinite_bits(unsigned u) { return (u & 0x7F800000u) == 0x7F800000u; }

// Four consecutive elements starting at 4 * q: one 16-byte load where the buffer allows it (VEC: base 16-byte aligned) and the
// quad is whole; returns how many of them exist
template <bool VEC>
__device__ __forceinline__ int load_quad(const float *d, long long q, long long n, float (&v)[4]) {
    const long long i = 4 * q;
    if (VEC && i + 3 < n) {
        const float4 t = *reinterpret_cast<const float4 *>(d + i);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        return 4;
    }
    int k = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const bool in = i + t < n;
        v[t] = in ? d[i + t] : 0.f;
        k += in ? 1 : 0;
    }
    return k;
}

// ---- distance pass: one item per (n, j), grid-stride over at most 4096 blocks ------------------------------------------------
__global__ __launch_bounds__(LB) void vertex_error_kernel(const float *pred, int ldp, const float *gt, const float *sd, const int *idx,
                                                          int N, int V, int Vc, float *dist, int row0) {
    const long long total = (long long)N * Vc;
    for (long long i = (long long)blockIdx.x * LB + threadIdx.x; i < total; i += (long long)gridDim.x * LB) {
        const int j = (int)(i % Vc);
        const long long n = i / Vc;
        const int v = idx[j];
        if ((unsigned)v >= (unsigned)V) {                          // an index outside the mesh: nothing is read, the count of
            dist[((long long)row0 + n) * Vc + j] = NAN;            // non-finite values shows it
            continue;
        }
        const float *p = pred + (n * V + v) * ldp, *g = gt + (n * V + v) * 3, *s = sd + (long long)v * 3;
        // the three differences and products in fp32 as the definition states them; the sum of squares and the root in fp64,
        // rounded once
        const float e0 = (p[0] - g[0]) * s[0], e1 = (p[1] - g[1]) * s[1], e2 = (p[2] - g[2]) * s[2];
        const double ss = (double)e0 * e0 + (double)e1 * e1 + (double)e2 * e2;
        dist[((long long)row0 + n) * Vc + j] = (float)sqrt(ss);
    }
}

// ---- moments ----------------------------------------------------------------------------------------------------------------
// one block per sample: the row's sum (thread-strided, then the block tree: a fixed order) and its non-finite count
__global__ __launch_bounds__(LB) void row_sum_kernel(const float *dist, int Vc, double *rowsum, unsigned *rownf, double *per_sample) {
    __shared__ double red[4];
    __shared__ unsigned redu[4];
    const float *row = dist + (long long)blockIdx.x * Vc;
    double s = 0.0;
    unsigned nf = 0;
    for (int j = threadIdx.x; j < Vc; j += LB) {
        const float v = row[j];
        s += (double)v;
        nf += nonfinite_bits(__float_as_uint(v)) ? 1u : 0u;
    }
    s = cape_block_sum256(s, red);
    nf = cape_block_sum256(nf, redu);
    if (threadIdx.x == 0) {
        rowsum[blockIdx.x] = s;
        rownf[blockIdx.x] = nf;
        per_sample[blockIdx.x] = s / (double)Vc;
    }
}

// one block: sum of `part` in a fixed order, divided by n; with `cnt`, the total count next to it (moments[2])
__global__ __launch_bounds__(LB) void final_kernel(const double *part, const unsigned *cnt, int nb, double n, double *out, double *out_cnt) {
    __shared__ double red[4];
    double s = 0.0, c = 0.0;                                   // counts: integers below 2^31, exact in fp64
    for (int i = threadIdx.x; i < nb; i += LB) {
        s += part[i];
        if (cnt) c += (double)cnt[i];
    }
    s = cape_block_sum256(s, red);
    if (cnt) c = cape_block_sum256(c, red);
    if (threadIdx.x == 0) {
        out[0] = s / n;
        if (cnt) out_cnt[0] = c;
    }
}

template <bool VEC>
__global__ __launch_bounds__(LB) void var_kernel(const float *dist, long long n, const double *mean, double *part) {
    __shared__ double red[4];
    const double m = *mean;
    const long long quads = (n + 3) / 4;
    double s = 0.0;
    for (long long q = (long long)blockIdx.x * LB + threadIdx.x; q < quads; q += (long long)gridDim.x * LB) {
        float v[4];
        const int k = load_quad<VEC>(dist, q, n, v);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t >= k) break;
            const double e = (double)v[t] - m;
            s += e * e;
        }
    }
    s = cape_block_sum256(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// 16 columns x 64 row lanes per block: lane r sums rows r, r + 64, ... of its column in order, then one thread per column adds
// the 64 sums in order.  One thread walking a whole column alone (57 waves, S loads each, one after the other) was not
// measured; an earlier form, 64 columns x 16 row lanes = 57 blocks, took 38.8 us on [2048, 3627], this one 15.1 us.
__global__ __launch_bounds__(PV_COLS *PV_ROWS) void per_vertex_kernel(const float *dist, int S, int Vc, double *per_vertex) {
    __shared__ double part[PV_ROWS][PV_COLS];
    const int c = threadIdx.x % PV_COLS, r = threadIdx.x / PV_COLS;
    const int j = blockIdx.x * PV_COLS + c;
    double s = 0.0;
    if (j < Vc)
        for (int row = r; row < S; row += PV_ROWS) s += (double)dist[(long long)row * Vc + j];
    part[r][c] = s;
    __syncthreads();
    if (r == 0 && j < Vc) {
        double t = 0.0;
        for (int k = 0; k < PV_ROWS; ++k) t += part[k][c];
        per_vertex[j] = t / (double)S;
    }
}

// ---- radix select -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LB) void select_init_kernel(Ranks ranks, int R, unsigned *state, unsigned *ghist) {
    for (int i = threadIdx.x; i < R * NBINS; i += LB) ghist[i] = 0u;
    if (threadIdx.x < MAXR) {
        const int r = threadIdx.x;
        state[ST_PREFIX + r] = 0u;
        state[ST_REMAIN + r] = r < R ? ranks.r[r] : 0u;
        state[ST_GROUP + r] = 0u;                              // no digit chosen yet: every rank shares the empty prefix
    }
}

// One digit pass.  Ranks whose prefixes so far are equal share one histogram (that of the first such rank, their group); the
// prefixes of different groups differ above the digit, so an element counts in at most one.  himask: the bits above the digit.
template <bool VEC>
__global__ __launch_bounds__(LB) void select_hist_kernel(const float *dist, long long n, int R, int shift, unsigned digit_mask,
                                                         unsigned himask, const unsigned *state, unsigned *ghist) {
    extern __shared__ unsigned lh[];                            // [R][NBINS]
    unsigned prefix[MAXR];
    bool leader[MAXR];
#pragma unroll
    for (int r = 0; r < MAXR; ++r) {
        prefix[r] = r < R ? state[ST_PREFIX + r] : 0u;
        leader[r] = r < R && state[ST_GROUP + r] == (unsigned)r;
    }
    for (int i = threadIdx.x; i < R * NBINS; i += LB) lh[i] = 0u;
    __syncthreads();
    const long long quads = (n + 3) / 4;
    for (long long q = (long long)blockIdx.x * LB + threadIdx.x; q < quads; q += (long long)gridDim.x * LB) {
        float v[4];
        const int k = load_quad<VEC>(dist, q, n, v);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t >= k) break;
            const unsigned u = __float_as_uint(v[t]);
            int g = -1;
#pragma unroll
            for (int r = 0; r < MAXR; ++r)
                if (leader[r] && ((u ^ prefix[r]) & himask) == 0u) g = r;
            if (g >= 0) atomicAdd(&lh[g * NBINS + ((u >> shift) & digit_mask)], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < R * NBINS; i += LB) {
        const unsigned c = lh[i];
        if (c) atomicAdd(&ghist[i], c);
    }
}

// One workgroup: per rank, the digit whose bin holds the remaining rank; prefix and remaining rank updated, the groups
// recomputed, the histogram cleared for the next pass; after the last pass the prefixes are the order statistics.
__global__ __launch_bounds__(LB) void select_scan_kernel(int R, int shift, int last, unsigned *state, unsigned *ghist, float *out_order) {
    constexpr int PER = NBINS / LB;                             // consecutive bins per thread
    __shared__ unsigned tsum[LB];
    __shared__ unsigned new_prefix[MAXR], new_remain[MAXR];
    if (threadIdx.x < MAXR) {                                   // (overwritten below for every rank; ordered by the loop's barriers)
        new_prefix[threadIdx.x] = state[ST_PREFIX + threadIdx.x];
        new_remain[threadIdx.x] = state[ST_REMAIN + threadIdx.x];
    }
    for (int r = 0; r < R; ++r) {
        const unsigned *h = ghist + state[ST_GROUP + r] * NBINS + threadIdx.x * PER;
        const unsigned rem = state[ST_REMAIN + r];
        unsigned c[PER], mine = 0u;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            c[k] = h[k];
            mine += c[k];
        }
        __syncthreads();                                        // the previous rank's readers of tsum are done
        tsum[threadIdx.x] = mine;
        __syncthreads();
        unsigned before = 0u;                                   // elements in the bins of the threads below this one
        for (int t = 0; t < (int)threadIdx.x; ++t) before += tsum[t];
        if (before <= rem && rem - before < mine) {             // exactly one thread: the bin holding the rank is among its own
            unsigned b = before;
            int dig = -1;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                if (dig < 0) {
                    if (rem - b < c[k]) dig = k;
                    else b += c[k];
                }
            }
            new_prefix[r] = state[ST_PREFIX + r] | ((unsigned)(threadIdx.x * PER + dig) << shift);
            new_remain[r] = rem - b;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < R * NBINS; i += LB) ghist[i] = 0u;
    if (threadIdx.x < R) {
        const int r = threadIdx.x;
        int g = r;
        for (int k = r - 1; k >= 0; --k)
            if (new_prefix[k] == new_prefix[r]) g = k;
        state[ST_PREFIX + r] = new_prefix[r];
        state[ST_REMAIN + r] = new_remain[r];
        state[ST_GROUP + r] = (unsigned)g;
        if (last) out_order[r] = __uint_as_float(new_prefix[r]);
    }
}

inline int64_t align8(int64_t b) { return (b + 7) & ~(int64_t)7; }

// workspace: [state | histogram R x NBINS | variance partials MAXB | row sums S | row non-finite counts S]
struct Layout {
    int64_t state, hist, varpart, rowsum, rownf, total;
};
inline Layout layout(int64_t S, int R) {
    Layout l;
    l.state = 0;
    l.hist = ST_WORDS * 4;
    l.varpart = align8(l.hist + (int64_t)R * NBINS * 4);
    l.rowsum = l.varpart + (int64_t)MAXB * 8;
    l.rownf = l.rowsum + S * 8;
    l.total = align8(l.rownf + S * 4);
    return l;
}

inline bool sizes_ok(int64_t S, int64_t Vc) { return S >= 1 && Vc >= 1 && S * Vc < ((int64_t)1 << 31); }

}  // namespace

extern "C" int cape_vertex_error(const float *pred, int32_t ldp, const float *gt, const float *std_, const int32_t *idx, int32_t N,
                                 int32_t V, int32_t Vc, float *dist, int32_t row0, int32_t S, void *stream) {
    if (!pred || !gt || !std_ || !idx || !dist) return CAPE_EINVAL;
    if (N < 1 || V < 1 || Vc < 1 || S < 1 || Vc > V || ldp < 3 || row0 < 0) return CAPE_EINVAL;
    if ((int64_t)row0 + N > S || !sizes_ok(S, Vc)) return CAPE_EINVAL;
    CAPE_LAUNCH(vertex_error_kernel, dim3(cape_grid_blocks((long long)N * Vc, LB, 4096)), dim3(LB), 0, (hipStream_t)stream, pred,
                ldp, gt, std_, idx, N, V, Vc, dist, row0);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

extern "C" int64_t cape_error_stats_workspace_bytes(int32_t S, int32_t Vc, int32_t R) {
    if (!sizes_ok(S, Vc) || R < 1 || R > MAXR) return CAPE_EINVAL;
    return layout(S, R).total;
}

extern "C" int cape_error_stats(const float *dist, int32_t S, int32_t Vc, const int64_t *ranks, int32_t R, double *out_moments,
                                float *out_order, double *per_vertex, double *per_sample, void *workspace, int64_t workspace_bytes,
                                void *stream) {
    if (!dist || !ranks || !out_moments || !out_order || !per_vertex || !per_sample || !workspace) return CAPE_EINVAL;
    if (!sizes_ok(S, Vc) || R < 1 || R > MAXR) return CAPE_EINVAL;
    const long long n = (long long)S * Vc;
    Ranks rk = {};
    for (int r = 0; r < R; ++r) {
        if (ranks[r] < 0 || ranks[r] >= n) return CAPE_EINVAL;
        rk.r[r] = (uint32_t)ranks[r];
    }
    if (((uintptr_t)workspace & 7) || ((uintptr_t)dist & 3)) return CAPE_EINVAL;
    const Layout l = layout(S, R);
    if (workspace_bytes < l.total) return CAPE_EWORKSPACE;
    char *ws = (char *)workspace;
    unsigned *state = (unsigned *)(ws + l.state), *ghist = (unsigned *)(ws + l.hist), *rownf = (unsigned *)(ws + l.rownf);
    double *varpart = (double *)(ws + l.varpart), *rowsum = (double *)(ws + l.rowsum);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = ((uintptr_t)dist & 15) == 0;
    const long long quads = (n + 3) / 4;

    CAPE_LAUNCH(row_sum_kernel, dim3(S), dim3(LB), 0, st, dist, Vc, rowsum, rownf, per_sample);
    CAPE_LAUNCH_CHECK();
    CAPE_LAUNCH(final_kernel, dim3(1), dim3(LB), 0, st, rowsum, rownf, S, (double)n, out_moments, out_moments + 2);
    CAPE_LAUNCH_CHECK();
    const int nv = cape_grid_blocks(quads, LB, MAXB);
    if (vec)
        CAPE_LAUNCH(var_kernel<true>, dim3(nv), dim3(LB), 0, st, dist, n, out_moments, varpart);
    else
        CAPE_LAUNCH(var_kernel<false>, dim3(nv), dim3(LB), 0, st, dist, n, out_moments, varpart);
    CAPE_LAUNCH_CHECK();
    CAPE_LAUNCH(final_kernel, dim3(1), dim3(LB), 0, st, varpart, (const unsigned *)nullptr, nv, (double)n, out_moments + 1,
                (double *)nullptr);
    CAPE_LAUNCH_CHECK();
    CAPE_LAUNCH(per_vertex_kernel, dim3((Vc + PV_COLS - 1) / PV_COLS), dim3(PV_COLS * PV_ROWS), 0, st, dist, S, Vc, per_vertex);
    CAPE_LAUNCH_CHECK();

    CAPE_LAUNCH(select_init_kernel, dim3(1), dim3(LB), 0, st, rk, R, state, ghist);
    CAPE_LAUNCH_CHECK();
    long long hb = (n + HIST_ITEMS - 1) / HIST_ITEMS;
    const int nh = (int)(hb > HIST_MAXB ? HIST_MAXB : hb);
    const size_t lds = (size_t)R * NBINS * sizeof(unsigned);
    const int shifts[3] = {21, 10, 0}, bits[3] = {11, 11, 10};
    for (int p = 0; p < 3; ++p) {
        const unsigned digit_mask = (1u << bits[p]) - 1u;
        const unsigned himask = p == 0 ? 0u : ~0u << (shifts[p] + bits[p]);
        if (vec)
            CAPE_LAUNCH(select_hist_kernel<true>, dim3(nh), dim3(LB), lds, st, dist, n, R, shifts[p], digit_mask, himask, state, ghist);
        else
            CAPE_LAUNCH(select_hist_kernel<false>, dim3(nh), dim3(LB), lds, st, dist, n, R, shifts[p], digit_mask, himask, state, ghist);
        CAPE_LAUNCH_CHECK();
        CAPE_LAUNCH(select_scan_kernel, dim3(1), dim3(LB), 0, st, R, shifts[p], p == 2 ? 1 : 0, state, ghist, out_order);
        CAPE_LAUNCH_CHECK();
    }
    return CAPE_OK;
}
