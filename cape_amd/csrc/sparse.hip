// The streaming sparse-operator family (gfx950): standalone operator application, several applications in one launch (with the
// fused activation gradient), the combine epilogue of the up-sampling layers, and the two backward-prep fusions.  All kernels
// read/write [N, M, ld] views with channels contiguous, fp32 or bf16 storage, and use 16-byte accesses whenever the views allow.
#include "common.h"
#include "views.h"

namespace {

// blocks per sample of the sparse kernels (256 work items = (row, channel quad) pairs each)
__host__ __device__ inline int spmm_bps(int Mo, int cq) { return (int)(((long long)Mo * cq + 255) / 256); }

#ifndef CAPE_SPMM_UNROLL_DEFAULT
#define CAPE_SPMM_UNROLL_DEFAULT 4
#endif
// Knob of the vector sparse kernels (A/B switch, read once; CAPE_SPMM_WIDE: views.h):
//   CAPE_SPMM_UNROLL = 0 (entry loop as written), 4 or 8 (entries in unrolled groups, see cape_gather_csr)
inline int spmm_unroll() {
    static const int u = getenv("CAPE_SPMM_UNROLL") ? atoi(getenv("CAPE_SPMM_UNROLL")) : CAPE_SPMM_UNROLL_DEFAULT;
    return u >= 8 ? 8 : u >= 4 ? 4 : 0;
}
// launch KERNEL<VW, T, U> with VW = 8 / 4 (wide) and U from the knob (hint4: rows of at most 4 entries -> groups of 4): every
// vector launch of this file goes through here
#define CAPE_LAUNCH_SP(KERNEL, T, wide, hint4, ...)                                  \
    do {                                                                             \
        const int u_ = (hint4 && spmm_unroll()) ? 4 : spmm_unroll();                 \
        if (wide) {                                                                  \
            if (u_ == 8) CAPE_LAUNCH((KERNEL<8, T, 8>), __VA_ARGS__);                \
            else if (u_ == 4) CAPE_LAUNCH((KERNEL<8, T, 4>), __VA_ARGS__);           \
            else CAPE_LAUNCH((KERNEL<8, T, 0>), __VA_ARGS__);                        \
        } else {                                                                     \
            if (u_ == 8) CAPE_LAUNCH((KERNEL<4, T, 8>), __VA_ARGS__);                \
            else if (u_ == 4) CAPE_LAUNCH((KERNEL<4, T, 4>), __VA_ARGS__);           \
            else CAPE_LAUNCH((KERNEL<4, T, 0>), __VA_ARGS__);                        \
        }                                                                            \
    } while (0)

// ---- one output row of an operator, VW channels: acc = sum_e va[e] * x[ci[e], c..c+VW-1] ------------------------------------
// GATHER_PLAIN:  the sum as it stands.
// GATHER_MASKED: every gathered row is multiplied by its own sign bits first (x_masked = bit ? x : 0).
// GATHER_BOTH:   the masked sum in acc AND the plain sum in acc_p from ONE set of loads (an up-sampling affine block applies S_0^T
//                to dz and to g).
// All three run the same fma chain over the same entries in the same order: acc of MASKED / BOTH is bit-identical to PLAIN on a
// pre-masked input, acc_p of BOTH to PLAIN.  acc_p is read and written in mode BOTH only (the other callers pass acc again).
enum { GATHER_PLAIN = 0, GATHER_MASKED = 1, GATHER_BOTH = 2 };

// sign bits of the gathered rows: word (row * words) of mb, channel c at bit sh (unused in mode PLAIN: pass {})
struct GatherMask {
    const unsigned *mb;
    int words, sh;
};

template <int VW>
__device__ __forceinline__ void cape_mask_row(float (&x)[VW], unsigned bits) {
#pragma unroll
    for (int u = 0; u < VW; ++u) x[u] = ((bits >> u) & 1u) ? x[u] : 0.f;
}

// CSR form.
// U = 0, PLAIN: entry loop as written -- the index load, then the row load that depends on it, then the next entry: two
// dependent memory round trips per entry.
// otherwise: entries in groups of U (of 1 for U = 0), fully unrolled: all (index, value) pairs of a group are loaded first, then
// all row gathers (and sign words) are in flight together, so a row of <= U entries costs three dependent round trips (row pointer,
// entries, rows).  Slots past the end of the row re-read its first entry with weight 0 (same address as slot 0: one L1 line)
// and add nothing; the order of the sum is unchanged.
template <int VW, int U, int MODE, typename T>
__device__ __forceinline__ void cape_gather_csr(const T *xb, long long ldx, GatherMask M, const int *rp, const int *ci, const float *va, int r,
                                                float (&acc)[VW], float (&acc_p)[VW]) {
#pragma unroll
    for (int u = 0; u < VW; ++u) {
        acc[u] = 0.f;
        if constexpr (MODE == GATHER_BOTH) acc_p[u] = 0.f;
    }
    int e = rp[r];
    const int e1 = rp[r + 1];
    if constexpr (U == 0 && MODE == GATHER_PLAIN) {
        for (; e < e1; ++e) {
            const float v = va[e];
            float xv[VW];
            cape_ldv<VW>(xb + (long long)ci[e] * ldx, xv);
#pragma unroll
            for (int u = 0; u < VW; ++u) acc[u] = fmaf(v, xv[u], acc[u]);
        }
    } else {
        constexpr int G = U > 0 ? U : 1;
        for (; e < e1; e += G) {
            int cols[G];
            float vals[G];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const bool ok = e + j < e1;
                const int ee = ok ? e + j : e;
                cols[j] = ci[ee];
                vals[j] = ok ? va[ee] : 0.f;
            }
            float xv[G][VW];
            unsigned mk[G];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                cape_ldv<VW>(xb + (long long)cols[j] * ldx, xv[j]);
                if constexpr (MODE != GATHER_PLAIN) mk[j] = M.mb[(long long)cols[j] * M.words] >> M.sh;
            }
#pragma unroll
            for (int j = 0; j < G; ++j) {
                if constexpr (MODE == GATHER_BOTH) {
#pragma unroll
                    for (int u = 0; u < VW; ++u) acc_p[u] = fmaf(vals[j], xv[j][u], acc_p[u]);
                }
                if constexpr (MODE != GATHER_PLAIN) cape_mask_row<VW>(xv[j], mk[j]);
#pragma unroll
                for (int u = 0; u < VW; ++u) acc[u] = fmaf(vals[j], xv[j][u], acc[u]);
            }
        }
    }
}

// ELL form of the same row (arrays [rows, ew], ew in {4, 8, 12}; entries in CSR order packed to the front, slots past the
// row's end hold (column of slot 0, 0.0f)): there is no row pointer to wait for, the index / value quads of the whole row
// are three independent 16-byte loads, and a row of <= 8 entries (every row of L~ but a handful) costs TWO dependent memory
// round trips instead of five (row pointer; per group of four: entries, rows).  These kernels are bound by exactly that
// chain times the occupancy (profiles/README.md), not by bytes.  Same entries in the same order as the CSR form: the sums
// are bit-identical.  An all-zero value quad ends the row (padding, or entries that contribute nothing).
template <int VW, int MODE, typename T>
__device__ __forceinline__ void cape_gather_ell(const T *xb, long long ldx, GatherMask M, const int *ec, const float *ev, int ew, int r,
                                                float (&acc)[VW], float (&acc_p)[VW]) {
#pragma unroll
    for (int u = 0; u < VW; ++u) {
        acc[u] = 0.f;
        if constexpr (MODE == GATHER_BOTH) acc_p[u] = 0.f;
    }
    const int4 *c4 = reinterpret_cast<const int4 *>(ec + (long long)r * ew);
    const float4 *v4 = reinterpret_cast<const float4 *>(ev + (long long)r * ew);
    int4 c0 = c4[0], c1 = c0, c2 = c0;
    float4 v0 = v4[0], v1 = make_float4(0.f, 0.f, 0.f, 0.f), v2 = v1;
    if (ew > 4) { c1 = c4[1]; v1 = v4[1]; }
    if (ew > 8) { c2 = c4[2]; v2 = v4[2]; }
    auto live = [](const float4 &v) { return v.x != 0.f || v.y != 0.f || v.z != 0.f || v.w != 0.f; };
    auto gather4 = [&](const int4 &c, float (&xv)[4][VW], unsigned (&mk)[4]) __attribute__((always_inline)) {
        cape_ldv<VW>(xb + (long long)c.x * ldx, xv[0]); cape_ldv<VW>(xb + (long long)c.y * ldx, xv[1]);
        cape_ldv<VW>(xb + (long long)c.z * ldx, xv[2]); cape_ldv<VW>(xb + (long long)c.w * ldx, xv[3]);
        if constexpr (MODE != GATHER_PLAIN) {
            mk[0] = M.mb[(long long)c.x * M.words] >> M.sh; mk[1] = M.mb[(long long)c.y * M.words] >> M.sh;
            mk[2] = M.mb[(long long)c.z * M.words] >> M.sh; mk[3] = M.mb[(long long)c.w * M.words] >> M.sh;
        }
    };
    auto fma4 = [&](const float4 &v, float (&xv)[4][VW], const unsigned (&mk)[4]) __attribute__((always_inline)) {
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (MODE == GATHER_BOTH) {
#pragma unroll
                for (int u = 0; u < VW; ++u) acc_p[u] = fmaf(vv[j], xv[j][u], acc_p[u]);
            }
            if constexpr (MODE != GATHER_PLAIN) cape_mask_row<VW>(xv[j], mk[j]);
#pragma unroll
            for (int u = 0; u < VW; ++u) acc[u] = fmaf(vv[j], xv[j][u], acc[u]);
        }
    };
    float xa[4][VW], xb2[4][VW];
    unsigned ma[4], mb2[4];
    const bool g1 = live(v1);
    gather4(c0, xa, ma);
    if (g1) gather4(c1, xb2, mb2);                // both groups in flight together
    fma4(v0, xa, ma);
    if (g1) {
        fma4(v1, xb2, mb2);
        if (live(v2)) {
            gather4(c2, xa, ma);
            fma4(v2, xa, ma);
        }
    }
}

// one output row, either form (ew = 0: CSR)
template <int VW, int U, int MODE, typename T>
__device__ __forceinline__ void cape_gather(const T *xb, long long ldx, GatherMask M, const int *rp, const int *ci, const float *va, int ew,
                                            int r, float (&acc)[VW], float (&acc_p)[VW]) {
    if (ew) cape_gather_ell<VW, MODE>(xb, ldx, M, ci, va, ew, r, acc, acc_p);
    else cape_gather_csr<VW, U, MODE>(xb, ldx, M, rp, ci, va, r, acc, acc_p);
}

// Row bound of an output (cape_store_rowmax): max |v[u]| over the cq lanes that hold the row -- consecutive and aligned, cq a power
// of two <= 64 (rm_fused) -- stored as row n * Mo + r by the lane that `store` names.  Dead lanes of a live block repeat the last
// row: same value.  (The row index is formed here, behind the predicate, as the call sites did: handed in ready-made it is hoisted
// ahead of the group maximum and the multi-term kernels are scheduled differently.)
template <int VW>
__device__ __forceinline__ void cape_row_bound(float *rm, const float (&v)[VW], int cq, int n, int Mo, int r, bool store) {
    float m = 0.f;
#pragma unroll
    for (int u = 0; u < VW; ++u) m = fmaxf(m, fabsf(v[u]));
    m = cape_group_max(m, cq);
    if (store) cape_store_rowmax(rm, (long long)n * Mo + r, m);
}

// Column sums over the rows of a 256-thread block, nterm <= MAXT terms of VW channels per lane, cq (a power of two, ROT4 ? >= 4 : >= 8,
// <= 64) lanes per row; a lane holds the same column group in every pass (256 % cq == 0).  Inside each wave over the lanes that hold
// the same column group without the LDS crossbar -- DPP row rotations by 4 (ROT4) and 8 inside the 16-lane rows, the 16- and 32-lane
// swaps across them -- then the four waves through LDS in a fixed order, all terms behind ONE barrier.  Term j goes to
// dst(j)[column]; dst captures by value (by reference the kernel arguments it names lose their no-clobber marking).  Every thread
// of the block must arrive.
// (first versions: ds_bpermute shuffles and a barrier pair per term, 5-7 us of a 21 us launch; cq threads adding 256 / cq LDS rows
// each, +10 us per launch)
template <int VW, int MAXT, bool ROT4, typename Dst>
__device__ __forceinline__ void cape_block_colsum(float (&s)[MAXT][VW], int nterm, int cq, Dst dst) {
    __shared__ float cs[4][MAXT][64 * VW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {
        if (j >= nterm) break;
#pragma unroll
        for (int u = 0; u < VW; ++u) {
            float v = s[j][u];
            if constexpr (ROT4)
                if (cq <= 4) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xF, 0xF, false));   // row_ror:4
            if (cq <= 8) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, false));   // row_ror:8
            if (cq <= 16) v = cape_sum_xor16(v);
            if (cq <= 32) v = cape_sum_xor32(v);
            s[j][u] = v;
        }
        if (lane < cq)
#pragma unroll
            for (int u = 0; u < VW; ++u) cs[wave][j][lane * VW + u] = s[j][u];
    }
    __syncthreads();
    if ((int)threadIdx.x < cq) {
#pragma unroll
        for (int j = 0; j < MAXT; ++j) {
            if (j >= nterm) break;
            float s4[VW];
#pragma unroll
            for (int u = 0; u < VW; ++u)
                s4[u] = ((cs[0][j][threadIdx.x * VW + u] + cs[1][j][threadIdx.x * VW + u]) + cs[2][j][threadIdx.x * VW + u]) + cs[3][j][threadIdx.x * VW + u];
            cape_stv<VW>(dst(j) + (int)threadIdx.x * VW, s4);
        }
    }
}

// ---- spmm: y[n,r,:] = alpha * S x[n] + beta * z[n,r,:] ------------------------------------
// work item = (sample, output row, VW channels); VW = 1 for unaligned / odd channel counts
template <int VW, typename T = float, int U = 0>
__global__ __launch_bounds__(256) void spmm_kernel(CViewT<T> x, const int *rp, const int *ci, const float *va, int ew,
                                                   float alpha, CViewT<T> z, float beta, ViewT<T> y, int N, int Mo, int C, float *rm) {
    const int cq = (C + VW - 1) / VW;
    // block -> (sample, 256 work items of that sample), all blocks of a sample on ONE XCD (spmm_grid / cape_map_block): the
    // ~7 neighbour rows an output row gathers are then served by the L2 that already holds that sample, instead of every
    // XCD fetching nearly the whole input (measured: 2.9x the algorithmic bytes in L2-miss traffic with linear blocks)
    int n, t;
    cape_map_block(blockIdx.x, N, spmm_bps(Mo, cq), n, t);
    const int i = t * 256 + (int)threadIdx.x;               // Mo * cq < 2^31 (checked by the host entry)
    if (i >= Mo * cq) return;
    const int r = i / cq;
    const int c = (i - r * cq) * VW;
    float acc[VW];
    cape_gather<VW, U, GATHER_PLAIN>(x.p + (long long)n * x.ss + c, x.ld, {}, rp, ci, va, ew, r, acc, acc);
#pragma unroll
    for (int u = 0; u < VW; ++u) acc[u] *= alpha;
    if (z.p) {
        float zv[VW];
        cape_ldv<VW>(z.p + (long long)n * z.ss + (long long)r * z.ld + c, zv);
#pragma unroll
        for (int u = 0; u < VW; ++u) acc[u] = fmaf(beta, zv[u], acc[u]);
    }
    cape_stv<VW>(y.p + (long long)n * y.ss + (long long)r * y.ld + c, acc);
    if (rm) cape_row_bound<VW>(rm, acc, cq, n, Mo, r, c == 0);
}

// ---- several operator applications in one launch -----------------------------------------------------------
// separate mode: y_k = S_k x_k for every term (the X_k = S_k x of one Chebyshev layer, or T_k = S_k^T dz of its
// data gradient);  sum mode: y = sum_k S_k x_k (dx = sum_k S_k^T G_k).  A term without CSR is the identity.
// One work item = (sample, output row, VW channels) of ALL terms: a layer pays one dispatch instead of K, and the
// terms' gathers of one neighbourhood hit the same L1/L2 lines.
struct SpmmTerms {
    struct T {
        const void *x; long long xs; int ldx;       // elements of the launch's storage type
        const int *rp; const int *ci; const float *va;      // ew > 0: ci / va are the ELL arrays [rows, ew]
        void *y; long long ys; int ldy;
        float scale;
        int ew;
        float *rm;                                  // row bounds of y (separate mode) or null
    } t[CAPE_MAX_SPMM_TERMS];
    int n;
};

// Sum mode with the activation gradient of the layer BELOW fused in (encoder chain, reference lib/models.py:154-171 cnp): the
// summed application is that layer's incoming gradient g; its own backward would next read g and its output x = act(z) once
// more to form dz = g * act'(x) and the channel-bias gradient sum_{n,r} dz (cape_bwd_prep: three tensor passes, one launch).
// Here the epilogue multiplies by act'(x) before the store and leaves the bias sums of the block's rows as partials in the
// layout cape_bwd_prep_finalize reads ([sample][block][2][C], term 0), so that layer needs no backward-prep launch at all.
struct SpmmActGrad {
    const void *ax; long long axs; int ldax;     // x = act(z) of the layer below: same rows / channels as the output; null = off
    int act;
    float *part;
};

template <int VW, typename T = float, int U = 0>
__global__ __launch_bounds__(256) void spmm_multi_kernel(SpmmTerms P, int sum, ViewT<T> y, int N, int Mo, int C, float *rm, SpmmActGrad G) {
    const int cq = (C + VW - 1) / VW;
    int n, t;
    cape_map_block(blockIdx.x, N, spmm_bps(Mo, cq), n, t);      // see spmm_kernel
    const int i = t * 256 + (int)threadIdx.x;
    const bool live = i < Mo * cq;
    if (!live && !G.ax) return;                             // (the fused form keeps whole blocks alive for its barrier)
    const int ii = live ? i : Mo * cq - 1;
    const int r = ii / cq;
    const int c = (ii - r * cq) * VW;
    float tot[VW];
#pragma unroll
    for (int u = 0; u < VW; ++u) tot[u] = 0.f;
    for (int k = 0; k < P.n; ++k) {
        const SpmmTerms::T &Tm = P.t[k];
        const T *xb = reinterpret_cast<const T *>(Tm.x) + (long long)n * Tm.xs + c;
        float acc[VW];
        if (!Tm.rp) cape_ldv<VW>(xb + (long long)r * Tm.ldx, acc);
        else cape_gather<VW, U, GATHER_PLAIN>(xb, Tm.ldx, {}, Tm.rp, Tm.ci, Tm.va, Tm.ew, r, acc, acc);
#pragma unroll
        for (int u = 0; u < VW; ++u) acc[u] *= Tm.scale;
        if (sum) {
#pragma unroll
            for (int u = 0; u < VW; ++u) tot[u] += acc[u];
        } else {
            cape_stv<VW>(reinterpret_cast<T *>(Tm.y) + (long long)n * Tm.ys + (long long)r * Tm.ldy + c, acc);
            if (Tm.rm) cape_row_bound<VW>(Tm.rm, acc, cq, n, Mo, r, c == 0);
        }
    }
    if (!sum) return;
    if (G.ax) {
        float xv[VW];
        cape_ldv<VW>(reinterpret_cast<const T *>(G.ax) + (long long)n * G.axs + (long long)r * G.ldax + c, xv);
#pragma unroll
        for (int u = 0; u < VW; ++u) tot[u] = live ? tot[u] * cape_act_grad_from_out(xv[u], G.act) : 0.f;
    }
    if (live) cape_stv<VW>(y.p + (long long)n * y.ss + (long long)r * y.ld + c, tot);
    if (rm) cape_row_bound<VW>(rm, tot, cq, n, Mo, r, live && c == 0);
    // the bias sums of the block's 256 / cq rows (cq >= 8: host check), term 0 of the partial layout
    if (G.ax)
        cape_block_colsum<VW, 1, false>(reinterpret_cast<float (&)[1][VW]>(tot), 1, cq,
                                        [=](int) { return G.part + (((long long)n * spmm_bps(Mo, cq) + t) * 2) * C; });
}

// ---- backward-prep of an affine block fused with the operator application of its data gradient ----------------------------
// res_block_affine at one resolution (reference lib/models.py:776-793: y = relu(conv_K(x)) + conv_1(x), K = 2), differentiated by
// tf.gradients (:460): the incoming gradient g feeds the 1x1 branch as it is and the K-branch as dz = g * [conv_K(x) > 0] (the
// sign bits the forward launch wrote); the data gradient then needs T_1 = L~^T dz next to dz itself, and the rank-1 condition
// terms need sum_r rowscale_j[r] dz[n,r,:] (j < R) and sum_r rowscale_rg[r] g[n,r,:].  cape_bwd_prep + cape_spmm did that in
// two launches and two more tensor passes; here one work item (sample, row, VW channels) writes dz of its row, gathers the
// MASKED neighbour rows of g for T_1 (x_masked = bit ? x : 0, then the same fma chain as cape_spmm: T_1 is bit-identical to
// the two-launch form), and the block reduces the weighted sums of its 256 / cq rows into the partial layout
// cape_bwd_prep_finalize reads ([sample][block][R + 2][C]; slot 0, the bias sum, is not written -- these blocks have no bias).
constexpr int PS_MAXR = 2;           // rank-1 terms of the fused form (K = 2); more: the caller keeps the two launches
struct PrepSpmmP {                      // g / dz / t1: elements of the launch's storage type (fp32 or bf16)
    const void *g; long long gs; int ldg;
    const unsigned *mask; int words;
    const int *rp; const int *ci; const float *va; int ew;
    void *dz; long long dzs; int lddz;
    void *t1; long long t1s; int ldt1;
    const float *rowscale; int R, rg;               // rg < 0: no g-weighted sum
    float *part;
    float *rm_g, *rm_t1;
};

// rpb: consecutive groups of 256 work items a block handles one after the other (the weighted sums of all of them are reduced
// ONCE: at 256 channels a group is only 8 rows, and one partial row per group and term would be a third of the tensor's bytes)
template <int VW, typename AT = float, int U = 0>
__global__ __launch_bounds__(256) void bwd_prep_spmm_kernel(PrepSpmmP P, int N, int Mo, int C, int rpb, int chunks) {
    const int cq = C / VW;                                   // a power of two in 4 .. 64 (host check): the lanes of a row are one aligned group
    int n, t;
    cape_map_block(blockIdx.x, N, chunks, n, t);             // see spmm_kernel
    const AT *gbase = reinterpret_cast<const AT *>(P.g) + (long long)n * P.gs;
    const unsigned *mbase = P.mask + (long long)n * Mo * P.words;
    const int nterm = P.R + (P.rg >= 0 ? 1 : 0);
    float racc[PS_MAXR + 1][VW];
#pragma unroll
    for (int j = 0; j <= PS_MAXR; ++j)
#pragma unroll
        for (int u = 0; u < VW; ++u) racc[j][u] = 0.f;
    for (int it = 0; it < rpb; ++it) {
        const int i = (t * rpb + it) * 256 + (int)threadIdx.x;
        const bool live = i < Mo * cq;                       // (whole blocks stay alive for the reductions)
        const int ii = live ? i : Mo * cq - 1;
        const int r = ii / cq;
        const int c = (ii - r * cq) * VW;
        const AT *gb = gbase + c;
        const unsigned *mb = mbase + (c >> 5);
        const int sh = c & 31;
        float gv[VW], d[VW], acc[VW];
        cape_ldv<VW>(gb + (long long)r * P.ldg, gv);
        const unsigned mw = mb[(long long)r * P.words] >> sh;
        // the row weights of the sums: loaded unconditionally on the clamped row, together with everything else (a guarded load
        // compiles to a branch with a wait for ALL outstanding loads in front of it: one more dependent round trip, +5 us)
        float sv[PS_MAXR + 1];
#pragma unroll
        for (int j = 0; j <= PS_MAXR; ++j) sv[j] = P.rowscale ? P.rowscale[(long long)(j == P.R ? (P.rg >= 0 ? P.rg : 0) : (j < P.R ? j : 0)) * Mo + r] : 0.f;
        cape_gather<VW, U, GATHER_MASKED>(gb, P.ldg, {mb, P.words, sh}, P.rp, P.ci, P.va, P.ew, r, acc, acc);
#pragma unroll
        for (int u = 0; u < VW; ++u) d[u] = gv[u];
        cape_mask_row<VW>(d, mw);
        if (live) {
            cape_stv<VW>(reinterpret_cast<AT *>(P.dz) + (long long)n * P.dzs + (long long)r * P.lddz + c, d);
            cape_stv<VW>(reinterpret_cast<AT *>(P.t1) + (long long)n * P.t1s + (long long)r * P.ldt1 + c, acc);
        }
        if (P.rm_t1) cape_row_bound<VW>(P.rm_t1, acc, cq, n, Mo, r, live && c == 0);
        if (P.rm_g) cape_row_bound<VW>(P.rm_g, gv, cq, n, Mo, r, live && c == 0);       // bounds g, and therefore dz
#pragma unroll
        for (int j = 0; j <= PS_MAXR; ++j)
            if (j < nterm) {
                const bool gterm = j == P.R;
                const float w = live ? sv[j] : 0.f;
#pragma unroll
                for (int u = 0; u < VW; ++u) racc[j][u] = fmaf(w, gterm ? gv[u] : d[u], racc[j][u]);
            }
    }
    // the weighted column sums of the block's rows: rank-1 term j -> slot 1 + j, the g-weighted sum -> slot R + 1.  This is
    // cape_block_colsum<VW, PS_MAXR + 1, true> written out: called through the helper, every instance of THIS kernel takes two more
    // vector registers (97 -> 99 at VW = 4, fp32; the bf16 4-wide form loses a wave per SIMD), whatever the helper's signature
    __shared__ float cs[4][PS_MAXR + 1][64 * VW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = P.R + 2;
    float *pp = P.part + ((long long)n * chunks + t) * T * C;
#pragma unroll
    for (int j = 0; j <= PS_MAXR; ++j) {
        if (j >= nterm) break;
#pragma unroll
        for (int u = 0; u < VW; ++u) {
            float v = racc[j][u];
            if (cq <= 4) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xF, 0xF, false));   // row_ror:4
            if (cq <= 8) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, false));   // row_ror:8
            if (cq <= 16) v = cape_sum_xor16(v);
            if (cq <= 32) v = cape_sum_xor32(v);
            racc[j][u] = v;
        }
        if (lane < cq)
#pragma unroll
            for (int u = 0; u < VW; ++u) cs[wave][j][lane * VW + u] = racc[j][u];
    }
    __syncthreads();
    if ((int)threadIdx.x < cq) {
#pragma unroll
        for (int j = 0; j <= PS_MAXR; ++j) {
            if (j >= nterm) break;
            const bool gterm = j == P.R;
            float s4[VW];
#pragma unroll
            for (int u = 0; u < VW; ++u)
                s4[u] = ((cs[0][j][threadIdx.x * VW + u] + cs[1][j][threadIdx.x * VW + u]) + cs[2][j][threadIdx.x * VW + u]) + cs[3][j][threadIdx.x * VW + u];
            cape_stv<VW>(pp + (long long)(gterm ? P.R + 1 : 1 + j) * C + (int)threadIdx.x * VW, s4);
        }
    }
}

// The same idea for the affine block that ALSO up-samples (reference lib/models.py:776-793 with an unpool in front, :147-151): its
// data gradient needs T_k = S_k^T dz (k < K) and T_aff = S_0^T g at the COARSE input rows, its weight gradient contracts those
// T_k (ChebConvFn coarse_dw), and the rank-1 condition sums are column sums of them:
//     sum_r (S_k 1)[r] dz[n,r,:] = sum_j (S_k^T dz)[n,j,:]
// so dz itself is needed by nobody.  cape_bwd_prep + cape_spmm_multi (separate mode) become ONE launch: every term gathers the
// fine rows of g, the terms flagged in `masked` multiply each gathered row by its sign bits first, and the block leaves the column
// sums of every term as partials in the cape_bwd_prep_finalize layout (term k -> slot 1 + k).
constexpr int MP_MAXT = 3;            // terms of cape_spmm_multi_prep (K = 2 orders + the affine term)
template <int VW, typename AT = float, int U = 0>
__global__ __launch_bounds__(256) void spmm_multi_prep_kernel(SpmmTerms P, unsigned masked, int pair, const unsigned *mask, int words, int Mfine,
                                                              int N, int Mo, int C, float *part, int T, int rpb, int chunks) {
    const int cq = C / VW;                                   // a power of two in 4 .. 64 (host check)
    int n, t;
    cape_map_block(blockIdx.x, N, chunks, n, t);             // see spmm_kernel
    const unsigned *mbase = mask + (long long)n * Mfine * words;
    float racc[MP_MAXT][VW];
#pragma unroll
    for (int k = 0; k < MP_MAXT; ++k)
#pragma unroll
        for (int u = 0; u < VW; ++u) racc[k][u] = 0.f;
    for (int it = 0; it < rpb; ++it) {
        const int i = (t * rpb + it) * 256 + (int)threadIdx.x;
        const bool live = i < Mo * cq;                       // (whole blocks stay alive for the reductions)
        const int ii = live ? i : Mo * cq - 1;
        const int r = ii / cq;
        const int c = (ii - r * cq) * VW;
        const unsigned *mb = mbase + (c >> 5);
        const int sh = c & 31;
        // `pair`: the last term applies the operator of term 0 to the same input, unmasked (T_aff = S_0^T g next to T_0 = S_0^T dz):
        // both from one set of gathered rows
        float accp[VW];
#pragma unroll
        for (int k = 0; k < MP_MAXT; ++k) {
            if (k >= P.n) break;
            const SpmmTerms::T &Tm = P.t[k];
            const AT *xb = reinterpret_cast<const AT *>(Tm.x) + (long long)n * Tm.xs + c;
            float acc[VW];
            if (pair && k == P.n - 1) {
#pragma unroll
                for (int u = 0; u < VW; ++u) acc[u] = accp[u];
            } else if (pair && k == 0) {
                cape_gather<VW, U, GATHER_BOTH>(xb, Tm.ldx, {mb, words, sh}, Tm.rp, Tm.ci, Tm.va, Tm.ew, r, acc, accp);
            } else if ((masked >> k) & 1u) {
                cape_gather<VW, U, GATHER_MASKED>(xb, Tm.ldx, {mb, words, sh}, Tm.rp, Tm.ci, Tm.va, Tm.ew, r, acc, acc);
            } else {
                cape_gather<VW, U, GATHER_PLAIN>(xb, Tm.ldx, {}, Tm.rp, Tm.ci, Tm.va, Tm.ew, r, acc, acc);
            }
            if (live) cape_stv<VW>(reinterpret_cast<AT *>(Tm.y) + (long long)n * Tm.ys + (long long)r * Tm.ldy + c, acc);
            if (Tm.rm) cape_row_bound<VW>(Tm.rm, acc, cq, n, Mo, r, live && c == 0);
#pragma unroll
            for (int u = 0; u < VW; ++u) racc[k][u] += live ? acc[u] : 0.f;
        }
    }
    if (!part) return;
    // the column sums of the block's rows: term k -> slot 1 + k
    float *pp = part + ((long long)n * chunks + t) * T * C;
    cape_block_colsum<VW, MP_MAXT, true>(racc, P.n, cq, [=](int k) { return pp + (long long)(1 + k) * C; });
}

// ---- operator applications AFTER the dense contraction (up-sampling layers) ----------------------------------
// (S_k x) W_k = S_k (x W_k): on an up-sampling layer the contraction runs on the coarse input rows (half the
// GEMM work) and this kernel applies the operators to the F-channel products Z_k, adds the rank-1 condition terms
// and performs the layer epilogue:   single:  y = act(acc1 + bias)      dual:  y = relu(acc1) + acc2, sign bits out
//   acc1 = sum_{k not in to2} S_k Z_k + sum_{j not in rank_to2} rowscale_j[r] coef[n,j,f];   acc2 likewise.
struct CombineParams {
    SpmmTerms P;
    unsigned to2;
    int rankR;
    const float *rowscale;
    const float *coef;
    unsigned rank_to2;
    const float *bias;
    int bias_mode, act, dual;
    unsigned *mask;
    int mask_words;
    float *rm;                                      // row bounds of y or null
};

template <int VW, typename T = float, int U = 0>
__global__ __launch_bounds__(256) void spmm_combine_kernel(CombineParams Q, ViewT<T> y, int N, int Mo, int F) {
    const int cq = (F + VW - 1) / VW;
    int n, t;
    cape_map_block(blockIdx.x, N, spmm_bps(Mo, cq), n, t);      // see spmm_kernel
    const int total = Mo * cq;                              // work items of one sample (< 2^31, checked by the host entry)
    const int i = t * 256 + (int)threadIdx.x;
    const bool live = i < total;                            // whole blocks stay alive: the mask shuffles need every lane
    const int ii = live ? i : total - 1;
    const int r = ii / cq;
    const int q = ii - r * cq;
    const int c = q * VW;
    float a1[VW], a2[VW];
#pragma unroll
    for (int u = 0; u < VW; ++u) a1[u] = a2[u] = 0.f;
    for (int k = 0; k < Q.P.n; ++k) {
        const SpmmTerms::T &Tm = Q.P.t[k];
        const T *xb = reinterpret_cast<const T *>(Tm.x) + (long long)n * Tm.xs + c;
        float acc[VW];
        if (!Tm.rp) cape_ldv<VW>(xb + (long long)r * Tm.ldx, acc);
        else cape_gather<VW, U, GATHER_PLAIN>(xb, Tm.ldx, {}, Tm.rp, Tm.ci, Tm.va, Tm.ew, r, acc, acc);
        if ((Q.to2 >> k) & 1u) {
#pragma unroll
            for (int u = 0; u < VW; ++u) a2[u] = fmaf(Tm.scale, acc[u], a2[u]);
        } else {
#pragma unroll
            for (int u = 0; u < VW; ++u) a1[u] = fmaf(Tm.scale, acc[u], a1[u]);
        }
    }
    for (int j = 0; j < Q.rankR; ++j) {
        const float rs = Q.rowscale[(long long)j * Mo + r];
        const float *cf = Q.coef + ((long long)n * Q.rankR + j) * F + c;
        if ((Q.rank_to2 >> j) & 1u) {
#pragma unroll
            for (int u = 0; u < VW; ++u) a2[u] = fmaf(rs, cf[u], a2[u]);
        } else {
#pragma unroll
            for (int u = 0; u < VW; ++u) a1[u] = fmaf(rs, cf[u], a1[u]);
        }
    }
    float o[VW];
    unsigned bits = 0;
#pragma unroll
    for (int u = 0; u < VW; ++u) {
        float v = a1[u];
        if (Q.dual) {
            if (v > 0.f) bits |= 1u << u;
            v = (v > 0.f ? v : 0.f) + a2[u];
        } else {
            if (Q.bias_mode == CAPE_BIAS_CHANNEL) v += Q.bias[c + u];
            else if (Q.bias_mode == CAPE_BIAS_VERTEX) v += Q.bias[(long long)r * F + c + u];
            v = cape_act(v, Q.act);
        }
        o[u] = v;
    }
    if (Q.mask) {
        // VW >= 4 only, F % 32 == 0: the 32 / VW lanes of one 32-channel word are consecutive and aligned
        constexpr int LW = VW >= 4 ? 32 / VW : 1;
        unsigned w = live ? (bits << (VW * (q & (LW - 1)))) : 0u;
#pragma unroll
        for (int s = 1; s < LW; s <<= 1) w |= __shfl_xor(w, s);
        if (live && (q & (LW - 1)) == 0) Q.mask[((long long)n * Mo + r) * Q.mask_words + (q / LW)] = w;
    }
    if (live) cape_stv<VW>(y.p + (long long)n * y.ss + (long long)r * y.ld + c, o);
    if (Q.rm) cape_row_bound<VW>(Q.rm, o, cq, n, Mo, r, live && c == 0);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// ELL operands: width 4, 8 or 12, 16-byte aligned arrays (0 = the operator is given in CSR form)
inline bool ell_ok(int ew, const void *ec, const void *ev) {
    if (ew == 0) return true;
    return (ew == 4 || ew == 8 || ew == 12) && ec && ev && ((reinterpret_cast<uintptr_t>(ec) | reinterpret_cast<uintptr_t>(ev)) & 15) == 0;
}

// Grid of the kernels that reduce over their rows (bwd_prep_spmm_kernel, spmm_multi_prep_kernel): a block handles rpb consecutive
// groups of 256 work items in turn (its sums are reduced once), chunks blocks per sample = partial rows per sample.  The *_chunks
// queries and the launches both ask here.  rpb was measured on the five affine-block shapes of the benchmarked step (16 samples,
// 108 groups each; tools/experiments/prep_spmm_bench.py under rocprofv3): 21.4 / 20.9 / 19.9 / 20.9 us at 1 / 2 / 3 / 4 -- three
// keeps 576 blocks for the 256 CUs
struct SpmmChunks {
    int rpb, chunks;
};
inline SpmmChunks chunks_for(int N, int Mo, int cq) {
    const int bps = spmm_bps(Mo, cq);
    const long long groups = (long long)N * bps;
    const int rpb = groups >= 1536 ? 3 : groups >= 1024 ? 2 : 1;
    return {rpb, (bps + rpb - 1) / rpb};
}

// What a kernel asks of every term it is handed (fill_terms):
enum {
    TERMS_Y = 1,            // each term has an output of its own: y is required and aligned like x, row bounds are allowed (fp32)
    TERMS_OPERATOR = 2,     // no identity terms
    TERMS_UNIT = 4          // scale == 1
};
struct TermsForm {
    bool vec, wide;         // every view of every term allows the 4-wide / the 8-wide form (wide: and the knob)
    bool any_ell;           // some operator is in ELL form (the scalar fallback reads CSR only)
};
// The kernel's SpmmTerms from the caller's cape_spmm_term_t[], checked; without TERMS_Y the terms' outputs and row bounds are left out
int fill_terms(SpmmTerms &P, const cape_spmm_term_t *terms, int nterms, int max_terms, int C, int es, unsigned flags, TermsForm &f) {
    if (!terms || nterms < 1 || nterms > max_terms) return CAPE_EINVAL;
    const bool ys = (flags & TERMS_Y) != 0;
    P.n = nterms;
    f.vec = true; f.wide = spmm_wide(); f.any_ell = false;
    for (int k = 0; k < nterms; ++k) {
        const cape_spmm_term_t &t = terms[k];
        if (!t.x || t.ldx < C) return CAPE_EINVAL;
        if (t.rowptr ? (!t.colidx || !t.vals || !ell_ok(t.ell_width, t.colidx, t.vals)) : (flags & TERMS_OPERATOR) != 0) return CAPE_EINVAL;
        if (ys && (!t.y || t.ldy < C || (t.rowmax_out && es != 4))) return CAPE_EINVAL;
        if ((flags & TERMS_UNIT) && t.scale != 1.0f) return CAPE_EINVAL;
        P.t[k].x = t.x; P.t[k].xs = t.x_sample_stride; P.t[k].ldx = t.ldx;
        P.t[k].rp = t.rowptr; P.t[k].ci = t.colidx; P.t[k].va = t.vals;
        P.t[k].y = ys ? t.y : nullptr; P.t[k].ys = ys ? t.y_sample_stride : 0; P.t[k].ldy = ys ? t.ldy : 0;
        P.t[k].scale = t.scale;
        P.t[k].ew = t.rowptr ? t.ell_width : 0;
        P.t[k].rm = ys ? t.rowmax_out : nullptr;
        f.any_ell = f.any_ell || P.t[k].ew;
        f.vec = f.vec && aligned4(t.x, t.x_sample_stride, t.ldx, C, es) && (!ys || aligned4(t.y, t.y_sample_stride, t.ldy, C, es));
        f.wide = f.wide && aligned8(t.x, t.x_sample_stride, t.ldx, C, es) && (!ys || aligned8(t.y, t.y_sample_stride, t.ldy, C, es));
    }
    f.wide = f.wide && f.vec;
    return CAPE_OK;
}

template <typename T>
int spmm_impl(const T *x, int64_t x_sample_stride, int32_t ldx, const int32_t *rowptr,
              const int32_t *colidx, const float *vals, int32_t max_row_nnz, int32_t ell_width, float alpha, const T *z,
              int64_t z_sample_stride, int32_t ldz, float beta, T *y, int64_t y_sample_stride,
              int32_t ldy, int32_t N, int32_t Mo, int32_t C, float *rowmax_out, void *stream) {
    if (!x || !rowptr || !colidx || !vals || !y || N < 1 || Mo < 1 || C < 1 || ldx < C || ldy < C) return CAPE_EINVAL;
    if (rowmax_out && sizeof(T) != 4) return CAPE_EINVAL;
    if (!ell_ok(ell_width, colidx, vals)) return CAPE_EINVAL;
    if (z && ldz < C) return CAPE_EINVAL;
    if ((long long)Mo * C >= (1LL << 31)) return CAPE_EINVAL;       // 32-bit work-item index per sample
    constexpr int es = (int)sizeof(T);
    CViewT<T> xv{x, x_sample_stride, ldx}, zv{z, z_sample_stride, ldz};
    ViewT<T> yv{y, y_sample_stride, ldy};
    const bool vec = aligned4(x, x_sample_stride, ldx, C, es) && aligned4(y, y_sample_stride, ldy, C, es) &&
                     (!z || aligned4(z, z_sample_stride, ldz, C, es));
    hipStream_t st = (hipStream_t)stream;
    if (vec) {
        // max_row_nnz is a hint: operators whose rows hold at most 4 entries (the up-/down-sampling matrices) take the
        // 4-wide entry groups
        const bool wide = spmm_wide() && aligned8(x, x_sample_stride, ldx, C, es) && aligned8(y, y_sample_stride, ldy, C, es) &&
                          (!z || aligned8(z, z_sample_stride, ldz, C, es));
        const bool hint4 = max_row_nnz >= 1 && max_row_nnz <= 4;
        float *rm = rm_fused(C / (wide ? 8 : 4)) ? rowmax_out : nullptr;
        CAPE_LAUNCH_SP(spmm_kernel, T, wide, hint4, dim3((unsigned)(N * spmm_bps(Mo, C / (wide ? 8 : 4)))), dim3(256), 0, st, xv, rowptr,
                       colidx, vals, ell_width, alpha, zv, beta, yv, N, Mo, C, rm);
        CAPE_LAUNCH_CHECK();
        if (rowmax_out && !rm) return rm_standalone(y, y_sample_stride, ldy, N, Mo, C, rowmax_out, stream);
        return CAPE_OK;
    } else {
        if (ell_width) return CAPE_EINVAL;                    // the scalar fallback reads CSR only
        CAPE_LAUNCH((spmm_kernel<1, T, 0>), dim3((unsigned)(N * spmm_bps(Mo, C))), dim3(256), 0, st, xv, rowptr, colidx, vals, 0, alpha, zv, beta, yv, N, Mo, C,
                    (float *)nullptr);
    }
    CAPE_LAUNCH_CHECK();
    if (rowmax_out) return rm_standalone(y, y_sample_stride, ldy, N, Mo, C, rowmax_out, stream);
    return CAPE_OK;
}
}  // namespace

extern "C" int cape_spmm(const float *x, int64_t x_sample_stride, int32_t ldx, const int32_t *rowptr,
                         const int32_t *colidx, const float *vals, int32_t max_row_nnz, int32_t ell_width, float alpha,
                         const float *z, int64_t z_sample_stride, int32_t ldz, float beta, float *y, int64_t y_sample_stride,
                         int32_t ldy, int32_t N, int32_t Mo, int32_t C, float *rowmax_out, void *stream) {
    return spmm_impl<float>(x, x_sample_stride, ldx, rowptr, colidx, vals, max_row_nnz, ell_width, alpha, z, z_sample_stride, ldz, beta, y,
                            y_sample_stride, ldy, N, Mo, C, rowmax_out, stream);
}

extern "C" int cape_spmm_bf16(const void *x, int64_t x_sample_stride, int32_t ldx, const int32_t *rowptr,
                              const int32_t *colidx, const float *vals, int32_t max_row_nnz, int32_t ell_width, float alpha,
                              const void *z, int64_t z_sample_stride, int32_t ldz, float beta, void *y, int64_t y_sample_stride,
                              int32_t ldy, int32_t N, int32_t Mo, int32_t C, float *rowmax_out, void *stream) {
    return spmm_impl<cape_bf16>((const cape_bf16 *)x, x_sample_stride, ldx, rowptr, colidx, vals, max_row_nnz, ell_width, alpha,
                                (const cape_bf16 *)z, z_sample_stride, ldz, beta, (cape_bf16 *)y, y_sample_stride, ldy, N, Mo, C,
                                rowmax_out, stream);
}

namespace {
template <typename T>
int spmm_multi_impl(const cape_spmm_term_t *terms, int32_t nterms, int32_t sum, T *y, int64_t y_sample_stride,
                    int32_t ldy, int32_t N, int32_t Mo, int32_t C, float *rowmax_out, void *stream, const SpmmActGrad *ag = nullptr) {
    if (N < 1 || Mo < 1 || C < 1) return CAPE_EINVAL;
    if (rowmax_out && (!sum || sizeof(T) != 4)) return CAPE_EINVAL;
    if (sum && (!y || ldy < C)) return CAPE_EINVAL;
    if ((long long)Mo * C >= (1LL << 31)) return CAPE_EINVAL;       // 32-bit work-item index per sample
    constexpr int es = (int)sizeof(T);
    SpmmTerms P;
    TermsForm f;
    if (fill_terms(P, terms, nterms, CAPE_MAX_SPMM_TERMS, C, es, sum ? 0 : TERMS_Y, f)) return CAPE_EINVAL;
    for (int k = 0; k < nterms && sum; ++k)
        if (terms[k].rowmax_out) return CAPE_EINVAL;            // sum mode has one output and one bound: rowmax_out
    const bool vec = f.vec && (!sum || aligned4(y, y_sample_stride, ldy, C, es));
    bool wide = f.wide && vec && (!sum || aligned8(y, y_sample_stride, ldy, C, es));
    const bool any_ell = f.any_ell;
    ViewT<T> yv{y, y_sample_stride, ldy};
    hipStream_t st = (hipStream_t)stream;
    SpmmActGrad G;
    G.ax = nullptr; G.axs = 0; G.ldax = 0; G.act = 0; G.part = nullptr;
    if (ag) {
        // the fused activation gradient: sum mode, vector form, the lanes of a row one aligned power-of-two group
        wide = wide && aligned8(ag->ax, ag->axs, ag->ldax, C, es);
        // (at least 8 lanes per row: the block reduction of the bias sums starts at the 8-lane rotation)
        if (!sum || !vec || !aligned4(ag->ax, ag->axs, ag->ldax, C, es) || !rm_fused(C / (wide ? 8 : 4)) || C / (wide ? 8 : 4) < 8 || !ag->part)
            return CAPE_EINVAL;
        G = *ag;
    }
    const bool fused = vec && rm_fused(C / (wide ? 8 : 4));
    if (!fused)
        for (int k = 0; k < nterms; ++k) P.t[k].rm = nullptr;
    if (vec) CAPE_LAUNCH_SP(spmm_multi_kernel, T, wide, false, dim3((unsigned)(N * spmm_bps(Mo, C / (wide ? 8 : 4)))), dim3(256), 0, st, P, sum, yv, N, Mo, C,
                            fused ? rowmax_out : (float *)nullptr, G);
    else if (any_ell) return CAPE_EINVAL;                      // the scalar fallback reads CSR only
    else CAPE_LAUNCH((spmm_multi_kernel<1, T, 0>), dim3((unsigned)(N * spmm_bps(Mo, C))), dim3(256), 0, st, P, sum, yv, N, Mo, C, (float *)nullptr, G);
    CAPE_LAUNCH_CHECK();
    if (!fused) {
        if (rowmax_out) {
            const int rc = rm_standalone(y, y_sample_stride, ldy, N, Mo, C, rowmax_out, stream);
            if (rc) return rc;
        }
        for (int k = 0; k < nterms && !sum; ++k)
            if (terms[k].rowmax_out) {
                const int rc = rm_standalone(reinterpret_cast<const T *>(terms[k].y), terms[k].y_sample_stride, terms[k].ldy, N, Mo, C,
                                             terms[k].rowmax_out, stream);
                if (rc) return rc;
            }
    }
    return CAPE_OK;
}
}  // namespace

extern "C" int cape_spmm_multi(const cape_spmm_term_t *terms, int32_t nterms, int32_t sum, float *y, int64_t y_sample_stride,
                               int32_t ldy, int32_t N, int32_t Mo, int32_t C, float *rowmax_out, void *stream) {
    return spmm_multi_impl<float>(terms, nterms, sum, y, y_sample_stride, ldy, N, Mo, C, rowmax_out, stream);
}

extern "C" int cape_spmm_multi_bf16(const cape_spmm_term_t *terms, int32_t nterms, int32_t sum, void *y, int64_t y_sample_stride,
                                    int32_t ldy, int32_t N, int32_t Mo, int32_t C, float *rowmax_out, void *stream) {
    return spmm_multi_impl<cape_bf16>(terms, nterms, sum, (cape_bf16 *)y, y_sample_stride, ldy, N, Mo, C, rowmax_out, stream);
}

// blocks per sample (= partial-sum chunks of the fused form) for a launch of C channels in the vector form it will take
static int actgrad_cq(const void *y, int64_t ys, int32_t ldy, const void *ax, int64_t axs, int32_t ldax, int32_t C, int es = 4) {
    const bool wide = spmm_wide() && aligned8(y, ys, ldy, C, es) && aligned8(ax, axs, ldax, C, es);
    return C / (wide ? 8 : 4);
}

extern "C" int32_t cape_spmm_multi_actgrad_chunks(const float *y, int64_t y_sample_stride, int32_t ldy, const float *act_x,
                                                  int64_t act_x_sample_stride, int32_t ld_act_x, int32_t Mo, int32_t C) {
    if (!y || !act_x || Mo < 1 || C < 4 || (C & 3)) return CAPE_EINVAL;
    const int cq = actgrad_cq(y, y_sample_stride, ldy, act_x, act_x_sample_stride, ld_act_x, C);
    if (cq < 8) return CAPE_EINVAL;                           // see spmm_multi_impl
    return spmm_bps(Mo, cq);
}

extern "C" int32_t cape_spmm_multi_actgrad_chunks_bf16(const void *y, int64_t y_sample_stride, int32_t ldy, const void *act_x,
                                                       int64_t act_x_sample_stride, int32_t ld_act_x, int32_t Mo, int32_t C) {
    if (!y || !act_x || Mo < 1 || C < 4 || (C & 3)) return CAPE_EINVAL;
    const int cq = actgrad_cq(y, y_sample_stride, ldy, act_x, act_x_sample_stride, ld_act_x, C, 2);
    if (cq < 8) return CAPE_EINVAL;                           // see spmm_multi_impl
    return spmm_bps(Mo, cq);
}

namespace {
template <typename T>
int spmm_multi_actgrad_impl(const cape_spmm_term_t *terms, int32_t nterms, T *y, int64_t y_sample_stride, int32_t ldy, int32_t N, int32_t Mo,
                            int32_t C, float *rowmax_out, const T *act_x, int64_t act_x_sample_stride, int32_t ld_act_x, int32_t act,
                            float *bias_partials, void *stream) {
    if (!act_x || !bias_partials || ld_act_x < C || (act != CAPE_ACT_LEAKY && act != CAPE_ACT_RELU)) return CAPE_EINVAL;
    // every term must allow the 8-wide form exactly when y and act_x do (the chunk count above assumes it)
    SpmmActGrad G;
    G.ax = act_x; G.axs = act_x_sample_stride; G.ldax = ld_act_x; G.act = act; G.part = bias_partials;
    const int cq = actgrad_cq(y, y_sample_stride, ldy, act_x, act_x_sample_stride, ld_act_x, C, (int)sizeof(T));
    for (int k = 0; k < nterms && terms; ++k)
        if (cq == C / 8 && !aligned8(terms[k].x, terms[k].x_sample_stride, terms[k].ldx, C, (int)sizeof(T))) return CAPE_EINVAL;
    return spmm_multi_impl<T>(terms, nterms, 1, y, y_sample_stride, ldy, N, Mo, C, rowmax_out, stream, &G);
}
}  // namespace

extern "C" int cape_spmm_multi_actgrad(const cape_spmm_term_t *terms, int32_t nterms, float *y, int64_t y_sample_stride, int32_t ldy,
                                       int32_t N, int32_t Mo, int32_t C, float *rowmax_out, const float *act_x,
                                       int64_t act_x_sample_stride, int32_t ld_act_x, int32_t act, float *bias_partials, void *stream) {
    return spmm_multi_actgrad_impl<float>(terms, nterms, y, y_sample_stride, ldy, N, Mo, C, rowmax_out, act_x, act_x_sample_stride, ld_act_x,
                                          act, bias_partials, stream);
}

extern "C" int cape_spmm_multi_actgrad_bf16(const cape_spmm_term_t *terms, int32_t nterms, void *y, int64_t y_sample_stride, int32_t ldy,
                                            int32_t N, int32_t Mo, int32_t C, float *rowmax_out, const void *act_x,
                                            int64_t act_x_sample_stride, int32_t ld_act_x, int32_t act, float *bias_partials, void *stream) {
    return spmm_multi_actgrad_impl<cape_bf16>(terms, nterms, (cape_bf16 *)y, y_sample_stride, ldy, N, Mo, C, rowmax_out,
                                              (const cape_bf16 *)act_x, act_x_sample_stride, ld_act_x, act, bias_partials, stream);
}

namespace {
template <typename T>
int spmm_combine_impl(const cape_spmm_term_t *terms, int32_t nterms, uint32_t to_acc2, const cape_rank_t *rank,
                      const float *bias, int32_t bias_mode, int32_t act, int32_t dual, uint32_t *mask_out, T *y,
                      int64_t y_sample_stride, int32_t ldy, int32_t N, int32_t Mo, int32_t F, float *rowmax_out, void *stream) {
    constexpr int es = (int)sizeof(T);
    if (rowmax_out && sizeof(T) != 4) return CAPE_EINVAL;
    if (!y || N < 1 || Mo < 1 || F < 1 || ldy < F) return CAPE_EINVAL;
    if (bias_mode != CAPE_BIAS_NONE && !bias) return CAPE_EINVAL;
    if (act < CAPE_ACT_NONE || act > CAPE_ACT_TANH) return CAPE_EINVAL;
    if (dual && (bias_mode != CAPE_BIAS_NONE || act != CAPE_ACT_NONE)) return CAPE_EINVAL;
    if (!dual && (to_acc2 || mask_out)) return CAPE_EINVAL;
    if ((long long)Mo * F >= (1LL << 31)) return CAPE_EINVAL;       // 32-bit work-item index per sample
    CombineParams Q;
    TermsForm f;
    if (fill_terms(Q.P, terms, nterms, CAPE_MAX_SPMM_TERMS, F, es, 0, f)) return CAPE_EINVAL;
    const bool vec = f.vec && aligned4(y, y_sample_stride, ldy, F, es);
    const bool wide = f.wide && vec && aligned8(y, y_sample_stride, ldy, F, es);
    const bool any_ell = f.any_ell;
    Q.to2 = to_acc2;
    Q.rankR = 0; Q.rowscale = nullptr; Q.coef = nullptr; Q.rank_to2 = 0;
    if (rank && rank->R > 0) {
        if (rank->R > CAPE_MAX_SRC || !rank->rowscale || !rank->coef || (rank->to_acc2 && !dual)) return CAPE_EINVAL;
        Q.rankR = rank->R; Q.rowscale = rank->rowscale; Q.coef = rank->coef; Q.rank_to2 = rank->to_acc2;
    }
    Q.bias = bias; Q.bias_mode = bias ? bias_mode : CAPE_BIAS_NONE; Q.act = act; Q.dual = dual ? 1 : 0;
    Q.mask = mask_out; Q.mask_words = (F + 31) / 32;
    if (mask_out && (!vec || (F & 31))) return CAPE_EINVAL;      // sign words are assembled from 8 float4 lanes
    ViewT<T> yv{y, y_sample_stride, ldy};
    hipStream_t st = (hipStream_t)stream;
    const bool fused = vec && rm_fused(F / (wide ? 8 : 4));
    Q.rm = fused ? rowmax_out : nullptr;
    if (vec) CAPE_LAUNCH_SP(spmm_combine_kernel, T, wide, false, dim3((unsigned)(N * spmm_bps(Mo, F / (wide ? 8 : 4)))), dim3(256), 0, st, Q, yv, N, Mo, F);
    else if (any_ell) return CAPE_EINVAL;
    else CAPE_LAUNCH((spmm_combine_kernel<1, T, 0>), dim3((unsigned)(N * spmm_bps(Mo, F))), dim3(256), 0, st, Q, yv, N, Mo, F);
    CAPE_LAUNCH_CHECK();
    if (rowmax_out && !fused) return rm_standalone(y, y_sample_stride, ldy, N, Mo, F, rowmax_out, stream);
    return CAPE_OK;
}
}  // namespace

extern "C" int cape_spmm_combine(const cape_spmm_term_t *terms, int32_t nterms, uint32_t to_acc2, const cape_rank_t *rank,
                                 const float *bias, int32_t bias_mode, int32_t act, int32_t dual, uint32_t *mask_out, float *y,
                                 int64_t y_sample_stride, int32_t ldy, int32_t N, int32_t Mo, int32_t F, float *rowmax_out, void *stream) {
    return spmm_combine_impl<float>(terms, nterms, to_acc2, rank, bias, bias_mode, act, dual, mask_out, y, y_sample_stride, ldy,
                                    N, Mo, F, rowmax_out, stream);
}

extern "C" int cape_spmm_combine_bf16(const cape_spmm_term_t *terms, int32_t nterms, uint32_t to_acc2, const cape_rank_t *rank,
                                      const float *bias, int32_t bias_mode, int32_t act, int32_t dual, uint32_t *mask_out, void *y,
                                      int64_t y_sample_stride, int32_t ldy, int32_t N, int32_t Mo, int32_t F, float *rowmax_out, void *stream) {
    return spmm_combine_impl<cape_bf16>(terms, nterms, to_acc2, rank, bias, bias_mode, act, dual, mask_out, (cape_bf16 *)y,
                                        y_sample_stride, ldy, N, Mo, F, rowmax_out, stream);
}

// work items per row of the fused backward-prep + operator application: 8 channels each where every view allows it, else 4;
// 0 = the arguments do not allow the fused form at all.  es = bytes per element (4: fp32, 2: bf16 storage)
static int prep_spmm_cq(const void *g, int64_t gs, int32_t ldg, const void *dz, int64_t dzs, int32_t lddz, const void *t1,
                        int64_t t1s, int32_t ldt1, int32_t F, int es) {
    if ((F & 31) || !aligned4(g, gs, ldg, F, es) || !aligned4(dz, dzs, lddz, F, es) || !aligned4(t1, t1s, ldt1, F, es)) return 0;
    const bool wide = spmm_wide() && aligned8(g, gs, ldg, F, es) && aligned8(dz, dzs, lddz, F, es) && aligned8(t1, t1s, ldt1, F, es);
    const int cq = F / (wide ? 8 : 4);
    return (rm_fused(cq) && cq >= 4) ? cq : 0;
}
static int32_t prep_spmm_chunks(const void *g, int64_t gs, int32_t ldg, const void *dz, int64_t dzs, int32_t lddz, const void *t1, int64_t t1s,
                                int32_t ldt1, int32_t N, int32_t Mo, int32_t F, int es) {
    const int cq = prep_spmm_cq(g, gs, ldg, dz, dzs, lddz, t1, t1s, ldt1, F, es);
    if (!cq || Mo < 1 || N < 1) return 0;
    return chunks_for(N, Mo, cq).chunks;
}

extern "C" int32_t cape_bwd_prep_spmm_chunks(const float *g, int64_t g_sample_stride, int32_t ldg, const float *dz,
                                             int64_t dz_sample_stride, int32_t lddz, const float *t1, int64_t t1_sample_stride,
                                             int32_t ldt1, int32_t N, int32_t Mo, int32_t F) {
    return prep_spmm_chunks(g, g_sample_stride, ldg, dz, dz_sample_stride, lddz, t1, t1_sample_stride, ldt1, N, Mo, F, 4);
}
extern "C" int32_t cape_bwd_prep_spmm_chunks_bf16(const void *g, int64_t g_sample_stride, int32_t ldg, const void *dz,
                                                  int64_t dz_sample_stride, int32_t lddz, const void *t1, int64_t t1_sample_stride,
                                                  int32_t ldt1, int32_t N, int32_t Mo, int32_t F) {
    return prep_spmm_chunks(g, g_sample_stride, ldg, dz, dz_sample_stride, lddz, t1, t1_sample_stride, ldt1, N, Mo, F, 2);
}

namespace {
template <typename T>
int bwd_prep_spmm_impl(const T *g, int64_t g_sample_stride, int32_t ldg, const uint32_t *mask, const int32_t *rowptr, const int32_t *colidx,
                       const float *vals, int32_t ell_width, T *dz, int64_t dz_sample_stride, int32_t lddz, T *t1, int64_t t1_sample_stride,
                       int32_t ldt1, const float *rowscale, int32_t R, int32_t rg, int32_t N, int32_t Mo, int32_t F, float *partials,
                       int64_t partials_bytes, float *rowmax_g_out, float *rowmax_t1_out, void *stream) {
    constexpr int es = (int)sizeof(T);
    if (!g || !mask || !rowptr || !colidx || !vals || !dz || !t1 || N < 1 || Mo < 1 || F < 1 || ldg < F || lddz < F || ldt1 < F)
        return CAPE_EINVAL;
    if ((rowmax_g_out || rowmax_t1_out) && es != 4) return CAPE_EINVAL;
    if (R < 0 || R > PS_MAXR || ((R > 0 || rg >= 0) && (!rowscale || !partials))) return CAPE_EINVAL;
    if (!ell_ok(ell_width, colidx, vals)) return CAPE_EINVAL;
    if ((long long)Mo * F >= (1LL << 31)) return CAPE_EINVAL;
    const int cq = prep_spmm_cq(g, g_sample_stride, ldg, dz, dz_sample_stride, lddz, t1, t1_sample_stride, ldt1, F, es);
    if (!cq) return CAPE_EINVAL;
    const int rpb = chunks_for(N, Mo, cq).rpb, chunks = chunks_for(N, Mo, cq).chunks;
    if ((R > 0 || rg >= 0) && partials_bytes < (int64_t)N * chunks * (R + 2) * F * (int64_t)sizeof(float)) return CAPE_EWORKSPACE;
    PrepSpmmP P;
    P.g = g; P.gs = g_sample_stride; P.ldg = ldg;
    P.mask = mask; P.words = (F + 31) / 32;
    P.rp = rowptr; P.ci = colidx; P.va = vals; P.ew = ell_width;
    P.dz = dz; P.dzs = dz_sample_stride; P.lddz = lddz;
    P.t1 = t1; P.t1s = t1_sample_stride; P.ldt1 = ldt1;
    P.rowscale = rowscale; P.R = R; P.rg = rg < 0 ? -1 : rg;
    P.part = partials;
    P.rm_g = rowmax_g_out; P.rm_t1 = rowmax_t1_out;
    const bool wide = cq * 8 == F;
    CAPE_LAUNCH_SP(bwd_prep_spmm_kernel, T, wide, false, dim3((unsigned)(N * chunks)), dim3(256), 0, (hipStream_t)stream, P, N, Mo, F, rpb, chunks);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}
}  // namespace

extern "C" int cape_bwd_prep_spmm(const float *g, int64_t g_sample_stride, int32_t ldg, const uint32_t *mask, const int32_t *rowptr,
                                  const int32_t *colidx, const float *vals, int32_t ell_width, float *dz, int64_t dz_sample_stride,
                                  int32_t lddz, float *t1, int64_t t1_sample_stride, int32_t ldt1, const float *rowscale, int32_t R,
                                  int32_t rg, int32_t N, int32_t Mo, int32_t F, float *partials, int64_t partials_bytes,
                                  float *rowmax_g_out, float *rowmax_t1_out, void *stream) {
    return bwd_prep_spmm_impl<float>(g, g_sample_stride, ldg, mask, rowptr, colidx, vals, ell_width, dz, dz_sample_stride, lddz, t1,
                                     t1_sample_stride, ldt1, rowscale, R, rg, N, Mo, F, partials, partials_bytes, rowmax_g_out, rowmax_t1_out,
                                     stream);
}
extern "C" int cape_bwd_prep_spmm_bf16(const void *g, int64_t g_sample_stride, int32_t ldg, const uint32_t *mask, const int32_t *rowptr,
                                       const int32_t *colidx, const float *vals, int32_t ell_width, void *dz, int64_t dz_sample_stride,
                                       int32_t lddz, void *t1, int64_t t1_sample_stride, int32_t ldt1, const float *rowscale, int32_t R,
                                       int32_t rg, int32_t N, int32_t Mo, int32_t F, float *partials, int64_t partials_bytes,
                                       float *rowmax_g_out, float *rowmax_t1_out, void *stream) {
    return bwd_prep_spmm_impl<cape_bf16>((const cape_bf16 *)g, g_sample_stride, ldg, mask, rowptr, colidx, vals, ell_width, (cape_bf16 *)dz,
                                         dz_sample_stride, lddz, (cape_bf16 *)t1, t1_sample_stride, ldt1, rowscale, R, rg, N, Mo, F, partials,
                                         partials_bytes, rowmax_g_out, rowmax_t1_out, stream);
}

// work items per row of cape_spmm_multi_prep (8 channels where every view allows it, else 4) and the kernel's terms; 0 = not possible
static int multi_prep_cq(SpmmTerms &P, const cape_spmm_term_t *terms, int32_t nterms, int32_t C, int es) {
    TermsForm f;
    if ((C & 31) || fill_terms(P, terms, nterms, MP_MAXT, C, es, TERMS_Y | TERMS_OPERATOR | TERMS_UNIT, f) || !f.vec) return 0;
    const int cq = C / (f.wide ? 8 : 4);
    return (rm_fused(cq) && cq >= 4) ? cq : 0;
}
static int32_t multi_prep_chunks(const cape_spmm_term_t *terms, int32_t nterms, int32_t N, int32_t Mo, int32_t C, int es) {
    SpmmTerms P;
    const int cq = multi_prep_cq(P, terms, nterms, C, es);
    if (!cq || Mo < 1 || N < 1) return 0;
    return chunks_for(N, Mo, cq).chunks;
}

extern "C" int32_t cape_spmm_multi_prep_chunks(const cape_spmm_term_t *terms, int32_t nterms, int32_t N, int32_t Mo, int32_t C) {
    return multi_prep_chunks(terms, nterms, N, Mo, C, 4);
}
extern "C" int32_t cape_spmm_multi_prep_chunks_bf16(const cape_spmm_term_t *terms, int32_t nterms, int32_t N, int32_t Mo, int32_t C) {
    return multi_prep_chunks(terms, nterms, N, Mo, C, 2);
}

namespace {
template <typename T>
int spmm_multi_prep_impl(const cape_spmm_term_t *terms, int32_t nterms, uint32_t masked_terms, const uint32_t *mask, int32_t mask_rows,
                         int32_t N, int32_t Mo, int32_t C, float *partials, int64_t partials_bytes, void *stream) {
    SpmmTerms P;
    const int cq = multi_prep_cq(P, terms, nterms, C, (int)sizeof(T));
    if (!cq || N < 1 || Mo < 1 || mask_rows < 1 || (masked_terms && !mask) || (masked_terms >> nterms)) return CAPE_EINVAL;
    if ((long long)Mo * C >= (1LL << 31)) return CAPE_EINVAL;
    const int rpb = chunks_for(N, Mo, cq).rpb, chunks = chunks_for(N, Mo, cq).chunks;
    const int T_ = nterms + 1;
    if (partials && partials_bytes < (int64_t)N * chunks * T_ * C * (int64_t)sizeof(float)) return CAPE_EWORKSPACE;
    const bool wide = cq * 8 == C;
    const int words = (C + 31) / 32;
    // the last term is the first one without its mask (same operator arrays, same input): one set of gathers serves both
    const cape_spmm_term_t &ta = terms[0], &tb = terms[nterms - 1];
    const int pair = nterms >= 2 && (masked_terms & 1u) && !((masked_terms >> (nterms - 1)) & 1u) && ta.x == tb.x &&
                     ta.x_sample_stride == tb.x_sample_stride && ta.ldx == tb.ldx && ta.rowptr == tb.rowptr && ta.colidx == tb.colidx &&
                     ta.vals == tb.vals && ta.ell_width == tb.ell_width;
    CAPE_LAUNCH_SP(spmm_multi_prep_kernel, T, wide, false, dim3((unsigned)(N * chunks)), dim3(256), 0, (hipStream_t)stream, P, masked_terms, pair, mask,
                   words, mask_rows, N, Mo, C, partials, T_, rpb, chunks);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}
}  // namespace

extern "C" int cape_spmm_multi_prep(const cape_spmm_term_t *terms, int32_t nterms, uint32_t masked_terms, const uint32_t *mask,
                                    int32_t mask_rows, int32_t N, int32_t Mo, int32_t C, float *partials, int64_t partials_bytes,
                                    void *stream) {
    return spmm_multi_prep_impl<float>(terms, nterms, masked_terms, mask, mask_rows, N, Mo, C, partials, partials_bytes, stream);
}
extern "C" int cape_spmm_multi_prep_bf16(const cape_spmm_term_t *terms, int32_t nterms, uint32_t masked_terms, const uint32_t *mask,
                                         int32_t mask_rows, int32_t N, int32_t Mo, int32_t C, float *partials, int64_t partials_bytes,
                                         void *stream) {
    return spmm_multi_prep_impl<cape_bf16>(terms, nterms, masked_terms, mask, mask_rows, N, Mo, C, partials, partials_bytes, stream);
}

