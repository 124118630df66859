// The trailing contraction of the Chebyshev mesh convolution (gfx950 / CDNA4, fp32 MFMA).
//
//   y[n, r, :] = epilogue( sum_s  x_s[n][r, :] @ B_s )
//
// Every source x_s is a plain [N, Mo, C] view: the operators S_k (a precomposed T_k(L~), T_k(L~)*U,
// D*T_k(L~) or a transpose of one of those) are applied beforehand by the streaming kernels of
// sparse.hip.  The kernels of this file are the GENERIC form of that contraction: they stage the
// A-tile [BM x 32] in LDS from rows of any alignment (channel-offset views, odd channel counts
// without row padding) and multiply on v_mfma_f32_32x32x2_f32 (exact fp32); sources that allow it
// take the pipelined kernels of gemm_plain.h / gemm_split.h / gemm_h2.h instead.
// Together they cover chebyshev5 (reference lib/models.py:69-103), the bias/activation
// epilogues (:105-127), res_block_affine in DUAL mode (:776-793) and -- with transposed weights --
// their data gradients.  The weight-gradient kernel (contraction over vertices) lives below.
#include "common.h"
#include "gconv_shared.h"
#include "gemm_plain.h"
#include "gemm_split.h"
#include "gemm_h2.h"
#include "narrow.h"
#include <stdlib.h>
#include <algorithm>
#include <vector>

namespace {

constexpr int KC_DEFAULT = 32;   // contraction chunk staged per iteration

// ---- A-tile staging: source rows -> LDS [ROWS][KC+4] -------------------------------------
template <int ROWS, int LDA, int KC, typename AT = float>
__device__ __forceinline__ void stage_rows(float *sA, const SrcDev &S, int n, int r0, int Mo,
                                            int c0, int tid) {
    constexpr int QPR = KC / 4;            // float4 columns per row of the chunk
    constexpr int RP = 256 / QPR;          // rows staged per pass
    const int q = tid % QPR;
    const int rl0 = tid / QPR;
    const int c = c0 + 4 * q;
    const AT *x0 = reinterpret_cast<const AT *>(S.x) + (long long)n * S.xs;
    const AT *xb = x0 + c;
    const int nvalid = S.C - c;   // channels available from c
    constexpr int P = ROWS / RP;
    if (S.vec && (nvalid >= 4 || (nvalid > 0 && c + 4 <= S.ldx) || nvalid <= 0)) {
        // aligned source: issue every load of the chunk before the first LDS store.  A row
        // padded to a multiple of 4 floats lets the last (partial) float4 be loaded whole; the lanes
        // beyond C are zeroed below (e.g. the 3-channel network input in a 4-float row).
        float4 v[P];
#pragma unroll
        for (int pass = 0; pass < P; ++pass) {
            const int r = r0 + rl0 + RP * pass;
            // unconditional load from a clamped (always valid) row, zeroed by a select afterwards:
            // a branch around each load would make hipcc wait vmcnt(0) per load (serialised round trips)
            const int rc = r < Mo ? r : Mo - 1;
            v[pass] = cape_ld4((nvalid > 0 ? xb : x0) + (long long)rc * S.ldx);
        }
#pragma unroll
        for (int pass = 0; pass < P; ++pass) {
            const bool ok = (r0 + rl0 + RP * pass) < Mo;
            float4 o = v[pass];
            o.x = (ok && nvalid > 0) ? o.x : 0.f; o.y = (ok && nvalid > 1) ? o.y : 0.f;
            o.z = (ok && nvalid > 2) ? o.z : 0.f; o.w = (ok && nvalid > 3) ? o.w : 0.f;
            *reinterpret_cast<float4 *>(&sA[(rl0 + RP * pass) * LDA + 4 * q]) = o;
        }
        return;
    }
#pragma unroll
    for (int pass = 0; pass < P; ++pass) {
        // unaligned rows, or the last (partial) float4 of an unpadded row: element by element
        const int rl = rl0 + RP * pass;
        const int r = r0 + rl;
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        if (r < Mo && nvalid > 0) {
            const AT *xr = xb + (long long)r * S.ldx;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (u < nvalid) a[u] = cape_ld(xr + u);
        }
        *reinterpret_cast<float4 *>(&sA[rl * LDA + 4 * q]) = make_float4(a[0], a[1], a[2], a[3]);
    }
}

// ---- B-tile staging: weights [KC x BN] with arbitrary (row, col) strides -> LDS [KC][BN+4]
// NT = number of staging threads (the loader half of the workgroup)
template <int BN, int LDB, int NT, int KC>
__device__ __forceinline__ void stage_weights(float *sB, const float *w, long long rs, long long cs,
                                               int C, int F, int c0, int f0, int tid) {
    if (cs == 1 && ((rs & 3) == 0) && ((F & 3) == 0) && ((reinterpret_cast<uintptr_t>(w) & 15) == 0)) {
        // output index contiguous in memory (forward weights): float4 along f
        constexpr int NL = (KC * (BN / 4) + NT - 1) / NT;
        float4 v[NL];
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + i * NT;
            const int j4 = idx % (BN / 4), kk = idx / (BN / 4);
            const int c = c0 + kk, f = f0 + 4 * j4;
            const int cc = c < C ? c : C - 1, fc = f < F ? f : 0;      // clamped, always valid
            v[i] = *reinterpret_cast<const float4 *>(w + cc * rs + fc);
        }
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + i * NT;
            const int j4 = idx % (BN / 4), kk = idx / (BN / 4);
            const bool ok = (c0 + kk < C) && (f0 + 4 * j4 < F);
            float4 o = v[i];
            o.x = ok ? o.x : 0.f; o.y = ok ? o.y : 0.f; o.z = ok ? o.z : 0.f; o.w = ok ? o.w : 0.f;
            if (idx < KC * (BN / 4)) *reinterpret_cast<float4 *>(&sB[kk * LDB + 4 * j4]) = o;
        }
    } else if (rs == 1 && ((cs & 3) == 0) && ((C & 3) == 0) && ((reinterpret_cast<uintptr_t>(w) & 15) == 0)) {
        // contraction index contiguous in memory (transposed weights, data gradient): float4 along c
        constexpr int NL = ((KC / 4) * BN + NT - 1) / NT;
        float4 v[NL];
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + i * NT;
            const int k4 = idx % (KC / 4), j = idx / (KC / 4);
            const int c = c0 + 4 * k4, f = f0 + j;
            const int cc = c < C ? c : 0, fc = f < F ? f : F - 1;      // clamped, always valid
            v[i] = *reinterpret_cast<const float4 *>(w + cc + fc * cs);
        }
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + i * NT;
            const int k4 = idx % (KC / 4), j = idx / (KC / 4);
            const bool ok = (c0 + 4 * k4 < C) && (f0 + j < F);
            if (idx < (KC / 4) * BN) {
                sB[(4 * k4 + 0) * LDB + j] = ok ? v[i].x : 0.f;
                sB[(4 * k4 + 1) * LDB + j] = ok ? v[i].y : 0.f;
                sB[(4 * k4 + 2) * LDB + j] = ok ? v[i].z : 0.f;
                sB[(4 * k4 + 3) * LDB + j] = ok ? v[i].w : 0.f;
            }
        }
    } else {
        const bool kmajor = (rs == 1 && cs != 1);
#pragma unroll 4
        for (int idx = tid; idx < KC * BN; idx += NT) {
            int kk, j;
            if (kmajor) {
                kk = idx & (KC - 1);
                j = idx / KC;
            } else {
                j = idx % BN;
                kk = idx / BN;
            }
            const int c = c0 + kk, f = f0 + j;
            float v = 0.f;
            if (c < C && f < F) v = w[c * rs + f * cs];
            sB[kk * LDB + j] = v;
        }
    }
}

// Workgroup = 4 waves; every wave stages its share of the [BM x KC] A chunk and the [KC x BN]
// weight chunk, then multiplies.  3-4 resident workgroups per CU overlap each other's staging and MFMA
// phases (measured faster here than a loader/MFMA wave split and than a register-prefetch pipeline, which
// cost occupancy here; aligned sources take the pipelined kernel of gemm_plain.h instead).
template <int BM, int BN, int WAVES_M, int WAVES_N, bool DUAL, int KC = KC_DEFAULT, typename AT = float>
__global__ __launch_bounds__(256, 4) void gconv_fwd_kernel(GconvParams p) {
    constexpr int LDA = KC + 4;
    constexpr int LDB = BN + 4;
    constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    constexpr int A_SZ = BM * LDA, B_SZ = KC * LDB;
    constexpr int BUF_SZ = A_SZ + (DUAL ? 2 : 1) * B_SZ;
    static_assert(WAVES_M * WAVES_N == 4, "4 MFMA waves per workgroup");
    static_assert(TM >= 1 && TN >= 1, "wave tile must hold at least one 32x32 MFMA tile");

    __shared__ __attribute__((aligned(16))) float smem[BUF_SZ];

    const int tid = threadIdx.x;
    const int ltid = tid;
    const int lane = tid & 63, wave = (tid >> 6) & 3;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int li = lane & 31, lh = lane >> 5;

    int n, t;
    cape_map_block(blockIdx.x, p.N, p.row_tiles * p.col_tiles, n, t);
    const int r0 = (t / p.col_tiles) * BM;
    const int f0 = (t % p.col_tiles) * BN;

    f32x16 acc[TM][TN];
    f32x16 acc2[DUAL ? TM : 1][DUAL ? TN : 1];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                acc[a][b][g] = 0.f;
                if (DUAL) acc2[a][b][g] = 0.f;
            }

    int total = 0;
    for (int si = 0; si < p.nsrc; ++si) total += (p.s[si].C + KC - 1) / KC;

    // loader cursor (source, channel offset) of the NEXT chunk to stage; consumer cursor of the
    // chunk being multiplied (only its source's w2 flag matters)
    int l_si = 0, l_c0 = 0;
    int c_si = 0, c_c0 = 0;

    auto stage = [&](int buf) {
        const SrcDev &S = p.s[l_si];
        float *sA = smem + buf * BUF_SZ;
        float *sB = sA + A_SZ;
        stage_rows<BM, LDA, KC, AT>(sA, S, n, r0, p.Mo, l_c0, ltid);
        stage_weights<BN, LDB, 256, KC>(sB, S.w, S.wrs, S.wcs, S.C, p.F, l_c0, f0, ltid);
        if (DUAL && S.w2) stage_weights<BN, LDB, 256, KC>(sB + B_SZ, S.w2, S.w2rs, S.w2cs, S.C, p.F, l_c0, f0, ltid);
        l_c0 += KC;
        if (l_c0 >= S.C) { l_c0 = 0; ++l_si; }
    };

    auto compute = [&](int buf) {
            const float *sA = smem + buf * BUF_SZ;
            const float *sB = sA + A_SZ;
            const float *sB2 = sB + B_SZ;
            const bool has2 = DUAL && (p.s[c_si].w2 != nullptr);
#pragma unroll
            for (int kb = 0; kb < KC / 8; ++kb) {
                // contraction index permutation: MFMA step u of this block of 8 uses physical
                // index kb*8 + 4*lh + u for lane-half lh (same mapping for A and B).
                float4 av[TM];
                float bv[TN][4];
#pragma unroll
                for (int a = 0; a < TM; ++a)
                    av[a] = *reinterpret_cast<const float4 *>(
                        &sA[(wm * WTM + a * 32 + li) * LDA + kb * 8 + 4 * lh]);
#pragma unroll
                for (int b = 0; b < TN; ++b)
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        bv[b][u] = sB[(kb * 8 + 4 * lh + u) * LDB + wn * WTN + b * 32 + li];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int a = 0; a < TM; ++a) {
                        const float af = (u == 0) ? av[a].x : (u == 1) ? av[a].y : (u == 2) ? av[a].z : av[a].w;
#pragma unroll
                        for (int b = 0; b < TN; ++b)
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bv[b][u], acc[a][b], 0, 0, 0);
                    }
                }
                if (DUAL && has2) {
                    float b2v[TN][4];
#pragma unroll
                    for (int b = 0; b < TN; ++b)
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            b2v[b][u] = sB2[(kb * 8 + 4 * lh + u) * LDB + wn * WTN + b * 32 + li];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
#pragma unroll
                        for (int a = 0; a < TM; ++a) {
                            const float af = (u == 0) ? av[a].x : (u == 1) ? av[a].y : (u == 2) ? av[a].z : av[a].w;
#pragma unroll
                            for (int b = 0; b < TN; ++b)
                                acc2[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, b2v[b][u], acc2[a][b], 0, 0, 0);
                        }
                    }
                }
            }
            c_c0 += KC;
            if (c_c0 >= p.s[c_si].C) { c_c0 = 0; ++c_si; }
    };

    for (int it = 0; it < total; ++it) {
        __syncthreads();
        stage(0);
        __syncthreads();
        compute(0);
    }

    gconv_epilogue<BM, BN, WAVES_M, WAVES_N, DUAL, AT>(p, acc, acc2, n, r0, f0, wm, wn, li, lh);
}

// =============================================================================================
// weight gradient:  dW_s[c, f] = sum_{n, r} A_s[n, r, c] * dz[n, r, f]
// Each workgroup owns one [CT x FT] tile of one source's dW and one (sample, row-range)
// slice of the vertex dimension; partials go to the workspace and are summed in a fixed order
// by dw_reduce_kernel (deterministic; no float atomics).
// =============================================================================================
template <int CT, int FT, typename AT = float>
__global__ __launch_bounds__(256, 4) void gconv_dw_kernel(DwParams p) {
    constexpr int RK = 32;
    constexpr int LDA = CT + 4, LDB = FT + 4;
    constexpr int WTM = CT / 2, WTN = FT / 2;
    constexpr int TM = WTM / 32, TN = WTN / 32;
    __shared__ __attribute__((aligned(16))) float smem[RK * LDA + RK * LDB];
    float *sA = smem;
    float *sB = smem + RK * LDA;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;

    const int ntiles = p.tile_off[p.nsrc];
    int tile, split;                                  // split = group * rsplit + rs
    if (!cape_map_dw_block(blockIdx.x, ntiles, p.ngroups * p.rsplit, tile, split)) return;
    const int grp = split / p.rsplit;
    const int rs = split % p.rsplit;
    const int n_begin = grp * p.samples_per_group;
    const int n_end = min(p.N, n_begin + p.samples_per_group);
    int si = 0;
    while (si + 1 < p.nsrc && tile >= p.tile_off[si + 1]) ++si;
    const SrcDev &S = p.s[si];
    const int lt = tile - p.tile_off[si];
    const int c0 = (lt / p.ftiles) * CT;
    const int f0 = (lt % p.ftiles) * FT;
    const int ra = rs * p.rows_per_split;
    const int rb = min(p.Mo, ra + p.rows_per_split);

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[a][b][g] = 0.f;

    for (int n = n_begin; n < n_end; ++n) {
    const AT *dzb = reinterpret_cast<const AT *>(((p.dz2_mask >> si) & 1u) ? p.dz2 : p.dz) + (long long)n * p.dzs;
    const AT *xb = reinterpret_cast<const AT *>(S.x) + (long long)n * S.xs;

    for (int rbase = ra; rbase < rb; rbase += RK) {
        __syncthreads();
        // A chunk: RK rows x CT channels
        if (S.vec && (((S.C & 3) == 0) || (((S.C + 3) & ~3) <= S.ldx))) {
            // aligned source: all loads first, clamped rows/columns + select (partial channel tiles
            // included: a float4 column is either entirely inside [0, C) or entirely outside)
            constexpr int NA = RK * (CT / 4) / 256;
            float4 va4[NA];
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int idx = tid + i * 256;
                const int rl = idx / (CT / 4), q = idx % (CT / 4);
                const int r = rbase + rl;
                const int rc = r < rb ? r : rb - 1;
                const int cc = (c0 + 4 * q) < S.C ? (c0 + 4 * q) : 0;
                va4[i] = cape_ld4(xb + (long long)rc * S.ldx + cc);
            }
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int idx = tid + i * 256;
                const int rl = idx / (CT / 4), q = idx % (CT / 4);
                const bool okr = (rbase + rl) < rb;
                const int nv = S.C - (c0 + 4 * q);       // valid lanes of this float4 column
                float4 o = va4[i];
                o.x = (okr && nv > 0) ? o.x : 0.f; o.y = (okr && nv > 1) ? o.y : 0.f;
                o.z = (okr && nv > 2) ? o.z : 0.f; o.w = (okr && nv > 3) ? o.w : 0.f;
                *reinterpret_cast<float4 *>(&sA[rl * LDA + 4 * q]) = o;
            }
        } else
        for (int idx = tid; idx < RK * (CT / 4); idx += 256) {
            const int rl = idx / (CT / 4), q = idx % (CT / 4);
            const int r = rbase + rl;
            const int c = c0 + 4 * q;
            const int nvalid = S.C - c;
            float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rb && nvalid > 0) {
                if (S.vec && nvalid >= 4) {
                    v4 = cape_ld4(xb + (long long)r * S.ldx + c);
                } else {
                    float a[4] = {0.f, 0.f, 0.f, 0.f};
                    const AT *xr = xb + (long long)r * S.ldx + c;
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (u < nvalid) a[u] = cape_ld(xr + u);
                    v4 = make_float4(a[0], a[1], a[2], a[3]);
                }
            }
            *reinterpret_cast<float4 *>(&sA[rl * LDA + 4 * q]) = v4;
        }
        // B chunk: RK rows of dz x FT channels
        if (p.dzvec && ((p.F & 3) == 0)) {
            constexpr int NB = RK * (FT / 4) / 256;
            float4 vb4[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int idx = tid + i * 256;
                const int rl = idx / (FT / 4), q = idx % (FT / 4);
                const int r = rbase + rl;
                const int rc = r < rb ? r : rb - 1;
                const int fc = (f0 + 4 * q) < p.F ? (f0 + 4 * q) : 0;
                vb4[i] = cape_ld4(dzb + (long long)rc * p.lddz + fc);
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int idx = tid + i * 256;
                const int rl = idx / (FT / 4), q = idx % (FT / 4);
                const bool ok = ((rbase + rl) < rb) && ((f0 + 4 * q) < p.F);
                float4 o = vb4[i];
                o.x = ok ? o.x : 0.f; o.y = ok ? o.y : 0.f; o.z = ok ? o.z : 0.f; o.w = ok ? o.w : 0.f;
                *reinterpret_cast<float4 *>(&sB[rl * LDB + 4 * q]) = o;
            }
        } else
        for (int idx = tid; idx < RK * (FT / 4); idx += 256) {
            const int rl = idx / (FT / 4), q = idx % (FT / 4);
            const int r = rbase + rl;
            const int f = f0 + 4 * q;
            const int nvalid = p.F - f;
            float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < rb && nvalid > 0) {
                const AT *zr = dzb + (long long)r * p.lddz + f;
                if (p.dzvec && nvalid >= 4) {
                    v4 = cape_ld4(zr);
                } else {
                    float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (u < nvalid) a[u] = cape_ld(zr + u);
                    v4 = make_float4(a[0], a[1], a[2], a[3]);
                }
            }
            *reinterpret_cast<float4 *>(&sB[rl * LDB + 4 * q]) = v4;
        }
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < RK / 8; ++kb) {
            float av[TM][4], bv[TN][4];
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int u = 0; u < 4; ++u) av[a][u] = sA[(kb * 8 + 4 * lh + u) * LDA + wm * WTM + a * 32 + li];
#pragma unroll
            for (int b = 0; b < TN; ++b)
#pragma unroll
                for (int u = 0; u < 4; ++u) bv[b][u] = sB[(kb * 8 + 4 * lh + u) * LDB + wn * WTN + b * 32 + li];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int b = 0; b < TN; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a][u], bv[b][u], acc[a][b], 0, 0, 0);
        }
    }
    }   // samples of this group

    // partial slab layout: [split][part_off[si] + c*F + f]
    float *out = p.ws + (long long)split * p.slab + p.part_off[si];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b) {
            const int f = f0 + wn * WTN + b * 32 + li;
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int c = c0 + wm * WTM + a * 32 + (g & 3) + 8 * (g >> 2) + 4 * lh;
                if (c < S.C && f < p.F) out[(long long)c * p.F + f] = acc[a][b][g];
            }
        }
}

struct DwReduceParams {
    float *w[CAPE_MAX_SRC];
    long long wrs[CAPE_MAX_SRC], wcs[CAPE_MAX_SRC];
    long long part_off[CAPE_MAX_SRC + 1];
    int nsrc, F, nsplit, accumulate;
    const float *ws;
    long long slab;
};

// block = 16 consecutive output elements x 16 split lanes; fixed summation order (deterministic)
__device__ __forceinline__ void dw_reduce_body(const DwReduceParams &p, long long block) {
    __shared__ float red[16][17];
    const long long total = p.part_off[p.nsrc];
    const int el = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const long long i = block * 16 + el;
    float sum = 0.f;
    if (i < total) {
        float s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int sp = sl;
        for (; sp + 48 < p.nsplit; sp += 64) {
            sum += p.ws[(long long)sp * p.slab + i];
            s1 += p.ws[(long long)(sp + 16) * p.slab + i];
            s2 += p.ws[(long long)(sp + 32) * p.slab + i];
            s3 += p.ws[(long long)(sp + 48) * p.slab + i];
        }
        for (; sp < p.nsplit; sp += 16) sum += p.ws[(long long)sp * p.slab + i];
        sum = (sum + s1) + (s2 + s3);
    }
    red[sl][el] = sum;
    __syncthreads();
    if (sl == 0 && i < total) {
        int si = 0;
        while (si + 1 < p.nsrc && i >= p.part_off[si + 1]) ++si;
        const long long loc = i - p.part_off[si];
        const long long c = loc / p.F, f = loc % p.F;
        float t = 0.f;
#pragma unroll
        for (int l = 0; l < 16; ++l) t += red[l][el];
        float *dst = p.w[si] + c * p.wrs[si] + f * p.wcs[si];
        *dst = p.accumulate ? (*dst + t) : t;
    }
}

__global__ __launch_bounds__(256) void dw_reduce_kernel(DwReduceParams p) { dw_reduce_body(p, blockIdx.x); }

// Vector form: thread = 4 consecutive output elements (one float4 of a weight-gradient row), all splits summed
// in order with four independent partial sums -- fully coalesced slab reads.  Needs F % 4 == 0, unit column
// stride and 16-byte aligned destinations (the layer weights in the gradient bucket).
__device__ __forceinline__ void dw_reduce_vec_body(const DwReduceParams &p, long long block) {
    const long long total4 = p.part_off[p.nsrc] >> 2;
    const long long q = block * 256 + threadIdx.x;
    if (q >= total4) return;
    const long long i = q << 2;
    const float4 *src = reinterpret_cast<const float4 *>(p.ws + i);
    const long long step = p.slab >> 2;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
    int sp = 0;
    for (; sp + 3 < p.nsplit; sp += 4) {
        const float4 v0 = src[(long long)sp * step], v1 = src[(long long)(sp + 1) * step];
        const float4 v2 = src[(long long)(sp + 2) * step], v3 = src[(long long)(sp + 3) * step];
        a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
        a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
        a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
        a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
    }
    for (; sp < p.nsplit; ++sp) {
        const float4 v0 = src[(long long)sp * step];
        a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
    }
    float4 t;
    t.x = (a0.x + a1.x) + (a2.x + a3.x); t.y = (a0.y + a1.y) + (a2.y + a3.y);
    t.z = (a0.z + a1.z) + (a2.z + a3.z); t.w = (a0.w + a1.w) + (a2.w + a3.w);
    int si = 0;
    while (si + 1 < p.nsrc && i >= p.part_off[si + 1]) ++si;
    const long long loc = i - p.part_off[si];
    const long long c = loc / p.F, f = loc % p.F;
    float4 *dst = reinterpret_cast<float4 *>(p.w[si] + c * p.wrs[si] + f);
    if (p.accumulate) {
        const float4 o = *dst;
        t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
    }
    *dst = t;
}

__global__ __launch_bounds__(256) void dw_reduce_vec_kernel(DwReduceParams p) { dw_reduce_vec_body(p, blockIdx.x); }

// The slab reductions of SEVERAL weight-gradient launches in one dispatch (their partial slabs stay in their workspaces
// until then): per layer the reduction is a ~5 us dispatch whose result is only needed at the end of the backward pass.
struct DwReduceBatch {
    DwReduceParams it[CAPE_MAX_DW_REDUCE_ITEMS];
    int blk_off[CAPE_MAX_DW_REDUCE_ITEMS + 1];
    int vec[CAPE_MAX_DW_REDUCE_ITEMS];
    int n;
};

__global__ __launch_bounds__(256) void dw_reduce_batch_kernel(DwReduceBatch B) {
    int i = 0;
    while (i + 1 < B.n && (int)blockIdx.x >= B.blk_off[i + 1]) ++i;
    const long long b = (long long)blockIdx.x - B.blk_off[i];
    if (B.vec[i]) dw_reduce_vec_body(B.it[i], b);       // (uniform per block)
    else dw_reduce_body(B.it[i], b);
}

// es = bytes per activation element (4: fp32, 2: bf16 storage)
inline bool src_ok(const cape_src_t &s) { return s.x && s.C > 0 && s.ldx >= s.C; }
inline void set_src(SrcDev &d, const cape_src_t &s, int es = 4) {
    d.x = s.x; d.xs = s.x_sample_stride; d.ldx = s.ldx; d.C = s.C;
    d.w = s.w; d.wrs = s.w_rs; d.wcs = s.w_cs;
    d.w2 = s.w2; d.w2rs = s.w2_rs; d.w2cs = s.w2_cs;
    d.vec = ((s.ldx & 3) == 0) && ((s.x_sample_stride & 3) == 0) && ((reinterpret_cast<uintptr_t>(s.x) & (4 * es - 1)) == 0);
    d.wh = d.wl = d.wh2 = d.wl2 = nullptr;
    d.wp = d.wp2 = 0;
    d.rm = nullptr;
    d.rmw = 0;
}
inline int fill_src(SrcDev &d, const cape_src_t &s, int es = 4) {
    if (!src_ok(s)) return CAPE_EINVAL;
    set_src(d, s, es);
    return CAPE_OK;
}

// fp16 two-piece operands of a launch (cape_h2_t, may be null): piece planes / row bounds per source, column scales, the
// row-bound output of the epilogue
inline int fill_h2(GconvParams &p, const cape_h2_t *h2, bool dual, int out_deinterleave) {
    p.wsi = p.wsi2 = nullptr;
    p.rm_out = nullptr;
    p.rm_out_w = 0;
    if (!h2) return CAPE_OK;
    if (h2->rowmax_out) {
        if (out_deinterleave > 1 || h2->rowmax_out_w < (p.F + 31) / 32 || (h2->rowmax_out_w & 3)) return CAPE_EINVAL;
        p.rm_out = h2->rowmax_out;
        p.rm_out_w = h2->rowmax_out_w;
    }
    if (!h2->src) return CAPE_OK;
    p.wsi = h2->wscale_inv;
    p.wsi2 = dual ? h2->w2scale_inv : nullptr;
    for (int i = 0; i < p.nsrc; ++i) {
        const cape_h2_src_t &h = h2->src[i];
        SrcDev &d = p.s[i];
        d.wh = h.w_hi; d.wl = h.w_lo; d.wp = h.w_pitch;
        d.wh2 = d.w2 ? h.w2_hi : nullptr; d.wl2 = d.w2 ? h.w2_lo : nullptr; d.wp2 = h.w2_pitch;
        d.rm = h.rowmax; d.rmw = h.rowmax_w;
    }
    return CAPE_OK;
}

struct DwPlan {
    int ct, ft, ctiles[CAPE_MAX_SRC], ftiles, ntiles, rsplit, rows_per_split, ngroups, samples_per_group;
    int vstart[CAPE_MAX_SRC + 1];      // plain kernel: virtual channel axis (see DwParams)
    long long slab;
};

// slots: workgroups the launch aims at.  512 = two per CU for the serial kernels (dw_split / dw_plain / dw_packed / generic: a
// second workgroup hides their staging phase); 256 = one per CU for the pipelined dw_h2_kernel, which overlaps its phases
// inside each wave -- half the partial slabs to write and to reduce: step 2.697 -> 2.670 ms in three alternating A/B pairs on one
// box, the kernel itself 33 -> 37 us (profiles/r05_exp_dw_slots.txt); the same setting costs the serial bf16 kernels 5 %.
constexpr int DW_SLOTS_SERIAL = 512, DW_SLOTS_PIPELINED = 256;
inline void plan_dw_splits(int N, int Mo, DwPlan &pl, int slots = DW_SLOTS_SERIAL) {
    // ONE round of workgroups (two per CU = 512 slots) with equal contraction lengths: split over the samples first
    // (the largest divisor of N that fits: every group gets the same number of samples), then the vertex range into
    // equal row blocks.  (An older rule rounded the split count UP, so the widest layers ran 672 workgroups of 24 chunks
    // on 512 slots -- one and a third rounds, groups of 6 / 6 / 4 samples -- where 512 of 27 chunks do: 50.7 -> 43.8 us.)
    int S = slots / pl.ntiles;            // (768 / 1024 slots for the smaller tiles measured slower)
    if (S < 1) S = 1;
    int ngroups = 1;
    for (int d = 1; d <= N && d <= S; ++d)
        if (N % d == 0) ngroups = d;
    const int maxr = (Mo + 127) / 128;
    int rsplit = S / ngroups;
    if (rsplit > maxr) rsplit = maxr;
    if (rsplit < 1) rsplit = 1;
    int rows = (Mo + rsplit - 1) / rsplit;
    rows = ((rows + 31) / 32) * 32;
    pl.rows_per_split = rows;
    pl.rsplit = (Mo + rows - 1) / rows;
    pl.samples_per_group = N / ngroups;
    pl.ngroups = ngroups;
}

// generic kernel: one [ct x ft] tile grid per source
inline void plan_dw(const cape_src_t *srcs, int nsrc, int N, int Mo, int F, DwPlan &pl) {
    int maxC = 0;
    for (int i = 0; i < nsrc; ++i) maxC = srcs[i].C > maxC ? srcs[i].C : maxC;
    pl.ct = (maxC <= 64) ? 64 : 128;
    pl.ft = (F <= 64) ? 64 : 128;
    pl.ftiles = (F + pl.ft - 1) / pl.ft;
    pl.ntiles = 0;
    pl.slab = 0;
    for (int i = 0; i < nsrc; ++i) {
        pl.ctiles[i] = (srcs[i].C + pl.ct - 1) / pl.ct;
        pl.ntiles += pl.ctiles[i] * pl.ftiles;
        pl.slab += (long long)srcs[i].C * F;
    }
    plan_dw_splits(N, Mo, pl);
}

// pipelined plain kernel: tiles over the virtual channel axis.  Sources that share dz are packed back to back, so
// the narrow layers (3 x 32 channels at 6890 vertices) run as ONE tile that reads dz once instead of three
// half-empty tiles; with dz2 in play every source starts on a tile boundary (a tile has one gradient operand).
inline void plan_dw_plain(const cape_src_t *srcs, int nsrc, int N, int Mo, int F, bool pack, DwPlan &pl) {
    int sumC = 0, maxC = 0;
    pl.slab = 0;
    for (int i = 0; i < nsrc; ++i) {
        sumC += srcs[i].C;
        maxC = srcs[i].C > maxC ? srcs[i].C : maxC;
        pl.slab += (long long)srcs[i].C * F;
    }
    const int span = pack ? sumC : maxC;
    const int n128 = (span + 127) / 128, n64 = (span + 63) / 64;
    pl.ft = (F <= 32) ? 32 : (F <= 64) ? 64 : 128;
    pl.ct = (pl.ft == 32 || n64 == 2 * n128) ? 128 : 64;      // 64-wide tiles only where they save MFMA work
    pl.ftiles = (F + pl.ft - 1) / pl.ft;
    int v = 0;
    for (int i = 0; i < nsrc; ++i) {
        if (!pack) v = (v + pl.ct - 1) / pl.ct * pl.ct;
        pl.vstart[i] = v;
        v += srcs[i].C;
    }
    pl.vstart[nsrc] = v;
    pl.ntiles = ((v + pl.ct - 1) / pl.ct) * pl.ftiles;
    plan_dw_splits(N, Mo, pl);
}

// Plain = float4-addressable rows.  A channel count that is not a multiple of 4 qualifies when the
// row is padded to one (ld >= round_up(C, 4)): the pad lane only feeds an output row that is never stored
// (the 3-channel network input / output layers).
inline bool dw_srcs_plain(const cape_src_t *srcs, int nsrc, int es = 4) {
    for (int i = 0; i < nsrc; ++i)
        if ((((srcs[i].C + 3) & ~3) > srcs[i].ldx) || (srcs[i].ldx & 3) || (srcs[i].x_sample_stride & 3) ||
            (reinterpret_cast<uintptr_t>(srcs[i].x) & (4 * es - 1)))
            return false;
    return true;
}


inline bool dw_dz_vec(const float *dz, int64_t dz_sample_stride, int32_t lddz, const float *dz2, int es = 4) {
    return ((lddz & 3) == 0) && ((dz_sample_stride & 3) == 0) && ((reinterpret_cast<uintptr_t>(dz) & (4 * es - 1)) == 0) &&
           (!dz2 || (reinterpret_cast<uintptr_t>(dz2) & (4 * es - 1)) == 0);
}

// row bounds of the weight gradient's operands (cape_h2_dw_t, may be null)
inline void fill_h2_dw(DwParams &p, const cape_h2_dw_t *h2) {
    p.dzrm = p.dz2rm = nullptr;
    p.dzrmw = p.dz2rmw = 0;
    if (!h2) return;
    for (int i = 0; i < p.nsrc; ++i) { p.s[i].rm = h2->src_rowmax[i]; p.s[i].rmw = h2->src_rowmax_w[i]; }
    p.dzrm = h2->dz_rowmax; p.dzrmw = h2->dz_rowmax_w;
    p.dz2rm = h2->dz2_rowmax; p.dz2rmw = h2->dz2_rowmax_w;
}

// One weight-gradient call as every extern "C" entry point receives it.  dz / dz2 are float or, with bf16, cape_bf16 storage
// (strides in elements); h2: row bounds of the operands or null; the plan queries leave accumulate and the workspace empty.
struct DwCall {
    const cape_src_t *srcs;
    int nsrc, N, Mo, F, accumulate;
    const float *dz, *dz2;
    int64_t dz_sample_stride;
    int32_t lddz;
    uint32_t dz2_mask;
    void *workspace;
    int64_t workspace_bytes;
    bool bf16;
    const cape_h2_dw_t *h2;
};

// Kernel family of one weight-gradient launch (pure function of the arguments): DW_GENERIC, DW_PLAIN, DW_PACKED (narrow
// sources sharing a tile) or DW_SPLIT (plain sources on the bf16 pipe).  Fills the tile plan.
inline int choose_dw(const DwCall &c, DwPlan &pl) {
    static const int dwp_on = getenv("CAPE_DW_PLAIN") ? atoi(getenv("CAPE_DW_PLAIN")) : 1;      // 0: A/B against the generic kernel
    const cape_src_t *srcs = c.srcs;
    const int nsrc = c.nsrc, N = c.N, Mo = c.Mo, F = c.F, es = c.bf16 ? 2 : 4;
    const bool two = c.dz2 && c.dz2_mask;
    const bool dzvec = dw_dz_vec(c.dz, c.dz_sample_stride, c.lddz, c.dz2, es);
    const bool plain = dwp_on && dzvec && (((F + 3) & ~3) <= c.lddz) && dw_srcs_plain(srcs, nsrc, es);
    int sumC = 0;
    bool c4 = true;
    for (int i = 0; i < nsrc; ++i) { c4 = c4 && (srcs[i].C & 3) == 0; sumC += srcs[i].C; }
    // packing pays where several sources fit ONE tile (narrow layers of the fine mesh levels)
    // (and the output is narrow: with F > 64 the single packed tile over-splits the rows -- measured 1.8x slower)
    const bool packs = plain && c4 && !two && nsrc > 1 && sumC <= 128 && F <= 64;
    if (c.bf16) {
        // bf16 storage: the split-pipe kernel with one plane where it applies (plain sources, whole float4-equivalent
        // columns, even F); the 3-channel ends take the pipelined fp32-MFMA kernels like the fp32 path (packed when
        // several narrow sources share a tile, plain otherwise); the generic kernel for everything else
        if (plain && c4 && (F & 1) == 0) {
            plan_dw(srcs, nsrc, N, Mo, F, pl);
            return DW_SPLIT;
        }
        if (packs) {
            plan_dw_plain(srcs, nsrc, N, Mo, F, true, pl);
            return DW_PACKED;
        }
        plan_dw(srcs, nsrc, N, Mo, F, pl);
        return plain ? DW_PLAIN : DW_GENERIC;
    }
    // un-packed plain launches run on the bf16 pipe (dw_split_kernel); CAPE_DW_BF16X6=0 keeps them on the fp32 MFMA
    static const int dws_on = getenv("CAPE_DW_BF16X6") ? atoi(getenv("CAPE_DW_BF16X6")) : CAPE_DW_BF16X6_DEFAULT;
    const bool dw_split = dws_on && plain && !packs && c4 && (F & 1) == 0;
    if (packs) plan_dw_plain(srcs, nsrc, N, Mo, F, true, pl);
    else plan_dw(srcs, nsrc, N, Mo, F, pl);
    return packs ? DW_PACKED : dw_split ? DW_SPLIT : plain ? DW_PLAIN : DW_GENERIC;
}

// Kernel choice of one forward launch (pure function of the arguments).
struct FwdPlan {
    int family;   // 4: plain sources with <= 8 input channels in total (fwd_narrow_in_kernel; plain epilogue only, else family 1)
                  // 0: generic staging for unaligned / unpadded sources (gconv_fwd_kernel), 1: pipelined plain GEMM (gemm_plain_kernel),
                  // 2: plain GEMM on the bf16 matrix pipe with exact three-way operand split (gemm_split_kernel)
                  // 3: plain GEMM as three fp16 products on two-piece operands (gemm_h2_kernel; needs cape_h2_t operands)
    int BM, BN;
    int layout;   // family 1: 1 = weights contraction-contiguous, 0 = output-contiguous
};

inline FwdPlan plan_fwd(const GconvParams &p, const cape_src_t *srcs, bool dual, bool bf16 = false) {
    FwdPlan pl;
    static const int gp_on = getenv("CAPE_GEMM_PLAIN") ? atoi(getenv("CAPE_GEMM_PLAIN")) : 1;   // 0: A/B against the generic kernel
    pl.layout = gp_on ? gp_weight_layout(p, dual) : -1;
    if (bf16) {
        // bf16 storage: the split-pipe kernel with one plane where its staging applies (plain sources of whole 32-channel
        // chunks whose rows can be read 8 elements = 16 bytes at a time, F >= 64), the generic kernel otherwise
        bool ok = pl.layout >= 0 && p.F >= 64;
        for (int i = 0; i < p.nsrc && ok; ++i) {
            const long long ws = srcs[i].w_cs > srcs[i].w_rs ? srcs[i].w_cs : srcs[i].w_rs;
            ok = (srcs[i].ldx & 7) == 0 && (srcs[i].x_sample_stride & 7) == 0 && (reinterpret_cast<uintptr_t>(srcs[i].x) & 15) == 0 &&
                 (long long)p.Mo * srcs[i].ldx < (1LL << 31) && (long long)p.F * ws < (1LL << 31) &&
                 srcs[i].C % GS_KC == 0 && srcs[i].C >= GS_KC;
        }
        if (ok) {
            pl.family = 2;
            gs_tile(dual, p.N, p.Mo, p.F, pl.BM, pl.BN);
            return pl;
        }
        pl.layout = -1;
    }
    for (int i = 0; i < p.nsrc && pl.layout >= 0; ++i) {
        const long long ws = srcs[i].w_cs > srcs[i].w_rs ? srcs[i].w_cs : srcs[i].w_rs;
        if ((long long)p.Mo * srcs[i].ldx >= (1LL << 31) || (long long)p.F * ws >= (1LL << 31)) pl.layout = -1;   // 32-bit offsets
    }
    if (pl.layout >= 0 && h2_eligible(p, dual)) {
        pl.family = 3;
        pl.layout = 1;                                  // the piece planes are contraction-contiguous in every launch form
        int ktot = 0;
        for (int i = 0; i < p.nsrc; ++i) ktot += p.s[i].C;
        h2_tile(dual, p.N, p.Mo, p.F, ktot, pl.BM, pl.BN);
        return pl;
    }
    if (pl.layout >= 0) {
        // CAPE_GEMM_BF16X6=0: keep every contraction on the exact-fp32 MFMA (A/B switch)
        static const int gs_on = getenv("CAPE_GEMM_BF16X6") ? atoi(getenv("CAPE_GEMM_BF16X6")) : CAPE_GEMM_BF16X6_DEFAULT;
        if (gs_on && gs_eligible(p, dual)) {
            pl.family = 2;
            gs_tile(dual, p.N, p.Mo, p.F, pl.BM, pl.BN);
            return pl;
        }
        // at most 8 input channels over all sources (the 3-channel network inputs): the narrow side in registers (narrow.h)
        static const int narrow_on = getenv("CAPE_NARROW") ? atoi(getenv("CAPE_NARROW")) : 1;
        int sumC = 0;
        for (int i = 0; i < p.nsrc; ++i) sumC += p.s[i].C;
        if (narrow_on && !dual && sumC <= NARROW_MAXC && (p.F & 3) == 0 && p.F >= 16 && p.F <= 256 &&
            (long long)p.N * p.Mo < (1LL << 31)) {
            pl.family = 4;
            pl.BM = 256 / narrow_lpr(p.F / 4); pl.BN = p.F;
            return pl;
        }
        pl.family = 1;
        gp_tile(dual, p.F, pl.BM, pl.BN);
        return pl;
    }
    pl.family = 0;
    pl.BN = (p.F <= 32) ? 32 : (p.F <= 64 || dual) ? 64 : 128;
    pl.BM = 128;
    // small meshes: 128-row tiles leave <= 2 workgroups per CU (no overlap partner while staging);
    // 64-row tiles double the resident workgroups at the price of re-reading the weight tile
    constexpr int bm64_below = 640;
    if (pl.BN == 128 && (long long)p.N * ((p.Mo + 127) / 128) * ((p.F + 127) / 128) < bm64_below) pl.BM = 64;
    return pl;
}

inline int fill_fwd_srcs(GconvParams &p, const cape_src_t *srcs, int nsrc, bool &dual, int es = 4) {
    dual = false;
    for (int i = 0; i < nsrc; ++i) {
        if (!srcs[i].w) return CAPE_EINVAL;
        int rc = fill_src(p.s[i], srcs[i], es);
        if (rc) return rc;
        dual = dual || (srcs[i].w2 != nullptr);
    }
    p.nsrc = nsrc;
    return CAPE_OK;
}

}  // namespace

namespace {

int gconv_fwd_plan_impl(const cape_src_t *srcs, int32_t nsrc, int32_t N, int32_t Mo, int32_t F, int32_t plan[4], bool bf16,
                        const cape_h2_t *h2 = nullptr) {
    if (!srcs || nsrc < 1 || nsrc > CAPE_MAX_SRC || N < 1 || Mo < 1 || F < 1 || !plan) return CAPE_EINVAL;
    GconvParams p;
    bool dual;
    int rc = fill_fwd_srcs(p, srcs, nsrc, dual, bf16 ? 2 : 4);
    if (rc) return rc;
    p.N = N; p.Mo = Mo; p.F = F;
    rc = fill_h2(p, bf16 ? nullptr : h2, dual, 0);
    if (rc) return rc;
    const FwdPlan pl = plan_fwd(p, srcs, dual, bf16);
    plan[0] = pl.family; plan[1] = pl.BM; plan[2] = pl.BN; plan[3] = pl.family ? pl.layout : 0;
    return CAPE_OK;
}

template <typename AT>
void launch_generic_fwd(const GconvParams &p, const FwdPlan &pl, bool dual, dim3 grid, hipStream_t st) {
    const dim3 block(256);
    if (!dual) {
        if (pl.BN == 32) CAPE_LAUNCH((gconv_fwd_kernel<128, 32, 4, 1, false, KC_DEFAULT, AT>), grid, block, 0, st, p);
        else if (pl.BN == 64) CAPE_LAUNCH((gconv_fwd_kernel<128, 64, 4, 1, false, KC_DEFAULT, AT>), grid, block, 0, st, p);
        else if (pl.BM == 64) CAPE_LAUNCH((gconv_fwd_kernel<64, 128, 2, 2, false, KC_DEFAULT, AT>), grid, block, 0, st, p);
        else CAPE_LAUNCH((gconv_fwd_kernel<128, 128, 2, 2, false, KC_DEFAULT, AT>), grid, block, 0, st, p);
    } else {
        if (pl.BN == 32) CAPE_LAUNCH((gconv_fwd_kernel<128, 32, 4, 1, true, KC_DEFAULT, AT>), grid, block, 0, st, p);
        else CAPE_LAUNCH((gconv_fwd_kernel<128, 64, 4, 1, true, KC_DEFAULT, AT>), grid, block, 0, st, p);
    }
}

int gconv_fwd_impl(const cape_src_t *srcs, int32_t nsrc, float *y, int64_t y_sample_stride,
                   int32_t ldy, int32_t N, int32_t Mo, int32_t F, const float *bias,
                   int32_t bias_mode, int32_t act, uint32_t *mask_out, const cape_rank_t *rank,
                   int32_t out_deinterleave, void *stream, bool bf16, const cape_h2_t *h2 = nullptr) {
    if (!srcs || nsrc < 1 || nsrc > CAPE_MAX_SRC || !y || N < 1 || Mo < 1 || F < 1) return CAPE_EINVAL;
    if (bf16 && h2) return CAPE_EINVAL;
    const int dK = out_deinterleave > 1 ? out_deinterleave : 1;
    const int dstride = dK > 1 ? ((F / dK + 3) & ~3) : 0;
    if (dK > 1 && (F % dK != 0 || mask_out || rank || ldy < dK * dstride)) return CAPE_EINVAL;
    if (dK == 1 && ldy < F) return CAPE_EINVAL;
    if (bias_mode != CAPE_BIAS_NONE && !bias) return CAPE_EINVAL;
    if (act < CAPE_ACT_NONE || act > CAPE_ACT_TANH) return CAPE_EINVAL;
    GconvParams p;
    bool dual;
    int rc = fill_fwd_srcs(p, srcs, nsrc, dual, bf16 ? 2 : 4);
    if (rc) return rc;
    if (mask_out && !dual) return CAPE_EINVAL;
    if (dual && (bias_mode != CAPE_BIAS_NONE || act != CAPE_ACT_NONE)) return CAPE_EINVAL;
    p.y = y; p.ys = y_sample_stride; p.ldy = ldy;
    p.N = N; p.Mo = Mo; p.F = F;
    p.bias = bias; p.bias_mode = bias ? bias_mode : CAPE_BIAS_NONE; p.act = act;
    p.mask = mask_out; p.mask_words = (F + 31) / 32;
    p.rankR = 0; p.rowscale = nullptr; p.coef = nullptr; p.rank_to2 = 0;
    p.deintK = dK; p.deint_stride = dstride;
    if (rank && rank->R > 0) {
        if (rank->R > CAPE_MAX_SRC || !rank->rowscale || !rank->coef) return CAPE_EINVAL;
        if (rank->to_acc2 && !dual) return CAPE_EINVAL;
        p.rankR = rank->R; p.rowscale = rank->rowscale; p.coef = rank->coef; p.rank_to2 = rank->to_acc2;
    }
    rc = fill_h2(p, h2, dual, dK);
    if (rc) return rc;
    FwdPlan pl = plan_fwd(p, srcs, dual, bf16);
    if (pl.family == 4) {
        // the narrow kernel has the plain epilogue (bias + activation, float4 stores); anything else takes the tile kernel
        const bool ok = !p.rankR && !p.mask && dK == 1 && !p.rm_out && (ldy & 3) == 0 && (y_sample_stride & 3) == 0 &&
                        (reinterpret_cast<uintptr_t>(y) & 15) == 0 && (!p.bias || (reinterpret_cast<uintptr_t>(p.bias) & 15) == 0);
        if (ok) {
            const int lpr = narrow_lpr(F / 4), RL = 256 / lpr;
            long long blocks = ((long long)N * Mo + 4 * RL - 1) / (4 * RL);       // four rows per thread and pass
            if (blocks > 1024) blocks = 1024;                                     // (per-block set-up: weights into LDS, pointer table)
            CAPE_LAUNCH(fwd_narrow_in_kernel, dim3((unsigned)blocks), dim3(256), (size_t)NARROW_MAXC * 4 * lpr * sizeof(float),
                        (hipStream_t)stream, p, lpr);
            CAPE_LAUNCH_CHECK();
            return CAPE_OK;
        }
        pl.family = 1;
        gp_tile(dual, p.F, pl.BM, pl.BN);
    }
    p.row_tiles = (Mo + pl.BM - 1) / pl.BM;
    p.col_tiles = (F + pl.BN - 1) / pl.BN;
    dim3 grid((unsigned)(N * p.row_tiles * p.col_tiles));
    hipStream_t st = (hipStream_t)stream;
    if (pl.family == 3) {
        h2_launch(p, dual, pl.BM, pl.BN, grid, st);
    } else if (pl.family == 2) {
        gs_launch(p, dual, pl.BM, pl.layout, bf16, grid, st);
    } else if (pl.family == 1) {
        gp_launch(p, dual, pl.BM, pl.BN, pl.layout, grid, st);
    } else if (bf16) {
        launch_generic_fwd<cape_bf16>(p, pl, dual, grid, st);
    } else {
        launch_generic_fwd<float>(p, pl, dual, grid, st);
    }
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

// =============================================================================================================
// Weight gradient, host side.  Every entry point turns its arguments into a DwCall; dw_resolve decides ONCE what that call runs
// (kernel, tiles and splits, kernel arguments, grid, workspace need, the slab reduction) and every consumer reads the resulting
// DwLaunch: the plan queries copy four integers out of it, the stages hand it to dw_contract and / or dw_reduce, the batched
// reduction and contraction collect their items'.  A new kernel registers as a DwKernelId, in dw_resolve and in dw_contract.
// =============================================================================================================
inline long long dw_workspace_need(const DwPlan &pl) { return pl.slab * pl.ngroups * pl.rsplit * (long long)sizeof(float); }

struct DwLaunch {
    int kernel;                        // DwKernelId
    bool bf16, v4;                     // storage type of the operands; DW_H2 only: the 16-byte-load instantiation
    DwPlan pl;                         // (DW_H2: split for DW_SLOTS_PIPELINED)
    DwParams p;
    unsigned grid;
    DwReduceParams rp;                 // the fixed-order slab reduction: its arguments, float4 form or not, blocks of 256 threads
    bool rvec;
    int rblocks;
};

// launchable = false (the plan queries): nothing is checked that only a launch needs -- the workspace, dz2 behind its mask, the
// sources' pointers and pitches -- and L describes the launch those arguments would get.
int dw_resolve(const DwCall &c, DwLaunch &L, bool launchable = true) {
    if (!c.srcs || c.nsrc < 1 || c.nsrc > CAPE_MAX_SRC || !c.dz || c.N < 1 || c.Mo < 1 || c.F < 1 || c.lddz < c.F) return CAPE_EINVAL;
    if (launchable && (!c.workspace || (c.dz2_mask && !c.dz2))) return CAPE_EINVAL;
    const int nsrc = c.nsrc, es = c.bf16 ? 2 : 4;
    DwPlan &pl = L.pl;
    DwParams &p = L.p;
    DwReduceParams &rp = L.rp;
    const int fam = choose_dw(c, pl);
    // the operands
    p.nsrc = nsrc;
    for (int i = 0; i < nsrc; ++i) set_src(p.s[i], c.srcs[i], es);
    p.dz = c.dz; p.dz2 = c.dz2; p.dz2_mask = c.dz2 ? c.dz2_mask : 0u; p.dzs = c.dz_sample_stride; p.lddz = c.lddz;
    p.dzvec = dw_dz_vec(c.dz, c.dz_sample_stride, c.lddz, c.dz2, es);
    p.N = c.N; p.Mo = c.Mo; p.F = c.F;
    fill_h2_dw(p, c.bf16 ? nullptr : c.h2);
    // the kernel: a narrow form where one applies, else the two-piece kernel for a DW_SPLIT launch whose operands all carry row
    // bounds.  One workgroup per CU (256 slots) for that pipelined kernel ONLY: the narrow kernels are serial ones and keep the
    // 512-slot plan whether or not the launch carries row bounds.
    L.bf16 = c.bf16;
    L.kernel = fam;
    if (const int narrow = dw_narrow_mode(p, fam, c.bf16)) {
        L.kernel = narrow;                                        // narrow.h: same splits and slabs, tile 0's workgroups do all sources
    } else if (fam == DW_SPLIT && h2_dw_eligible(p)) {
        L.kernel = DW_H2;                                         // fp16 two-piece operands: same tiles and slabs, fewer splits
        plan_dw_splits(c.N, c.Mo, pl, DW_SLOTS_PIPELINED);
    }
    L.v4 = L.kernel == DW_H2 && h2_dw_v4(p, pl.ct, pl.ft);
    // tiles, splits and slabs
    const bool packed = fam == DW_PACKED;
    int toff = 0;
    long long poff = 0;
    for (int i = 0; i <= nsrc; ++i) {
        p.tile_off[i] = toff; p.part_off[i] = rp.part_off[i] = poff;
        p.vstart[i] = packed ? pl.vstart[i] : 0;
        if (i == nsrc) break;
        toff += packed ? 0 : pl.ctiles[i] * pl.ftiles;
        poff += (long long)c.srcs[i].C * c.F;
    }
    p.ftiles = pl.ftiles;
    p.rsplit = pl.rsplit; p.rows_per_split = pl.rows_per_split;
    p.ngroups = pl.ngroups; p.samples_per_group = pl.samples_per_group;
    p.ws = (float *)c.workspace; p.slab = pl.slab;
    L.grid = (unsigned)(pl.ntiles * ((pl.ngroups * pl.rsplit + 7) / 8) * 8);                  // cape_map_dw_block
    if (launchable) {
        if (c.workspace_bytes < dw_workspace_need(pl)) return CAPE_EWORKSPACE;
        for (int i = 0; i < nsrc; ++i)
            if (!c.srcs[i].w || !src_ok(c.srcs[i])) return CAPE_EINVAL;
    }
    // the slab reduction.  The float4 form sums a quad's splits serially: only when the slab alone fills the chip (>= 256 blocks
    // of quads); small slabs with many splits (fine mesh levels) take the kernel that also spreads the splits over 16 lanes
    rp.nsrc = nsrc; rp.F = c.F; rp.nsplit = pl.ngroups * pl.rsplit; rp.accumulate = c.accumulate;
    rp.ws = (const float *)c.workspace; rp.slab = pl.slab;
    L.rvec = (c.F & 3) == 0 && (pl.slab & 3) == 0 && (reinterpret_cast<uintptr_t>(c.workspace) & 15) == 0 && poff >= 262144;
    for (int i = 0; i < nsrc; ++i) {
        const cape_src_t &s = c.srcs[i];
        rp.w[i] = const_cast<float *>(s.w); rp.wrs[i] = s.w_rs; rp.wcs[i] = s.w_cs;
        L.rvec = L.rvec && s.w_cs == 1 && (s.w_rs & 3) == 0 && (reinterpret_cast<uintptr_t>(s.w) & 15) == 0;
    }
    L.rblocks = L.rvec ? (int)((poff / 4 + 255) / 256) : (int)((poff + 15) / 16);
    return CAPE_OK;
}

// The tile kernels (DW_GENERIC .. DW_SPLIT) for storage type AT: ONE ladder over the four square tiles; only dw_packed has a 32-wide one
using DwKernelFn = void (*)(DwParams);
template <typename AT>
DwKernelFn dw_tile_kernel(int kernel, int ct, int ft) {
#define DW_TILES(K, ...)                                                                                                    \
    (ct == 64 && ft == 64 ? DwKernelFn(K<64, 64, __VA_ARGS__>) : ct == 64 ? DwKernelFn(K<64, 128, __VA_ARGS__>)              \
     : ft == 64           ? DwKernelFn(K<128, 64, __VA_ARGS__>) : DwKernelFn(K<128, 128, __VA_ARGS__>))
    switch (kernel) {
    case DW_PACKED: return ft == 32 ? DwKernelFn(dw_packed_kernel<128, 32, 4, 1, AT>) : DW_TILES(dw_packed_kernel, 2, 2, AT);
    case DW_SPLIT: return DW_TILES(dw_split_kernel, AT);
    case DW_PLAIN: return DW_TILES(dw_plain_kernel, 2, 2, AT);
    default: return DW_TILES(gconv_dw_kernel, AT);
    }
#undef DW_TILES
}

// the contraction: partial slabs into the workspace
int dw_contract(const DwLaunch &L, hipStream_t st) {
    const DwParams &p = L.p;
    const dim3 grid(L.grid), block(256);
    if (L.kernel == DW_NARROW_IN) {
        CAPE_LAUNCH(dw_narrow_in_kernel, grid, block, 32768, st, p, narrow_lpr(p.F / 4), L.pl.ntiles);
    } else if (L.kernel == DW_NARROW_OUT) {
        const int sumC = (int)(p.part_off[p.nsrc] / p.F);
        CAPE_LAUNCH(dw_narrow_out_kernel, grid, block, 16384, st, p, narrow_lpr(sumC / 4), L.pl.ntiles);
    } else if (L.kernel == DW_H2) {
        h2_dw_launch(p, L.pl.ct, L.pl.ft, L.v4, grid, st);
    } else {
        const DwKernelFn k = L.bf16 ? dw_tile_kernel<cape_bf16>(L.kernel, L.pl.ct, L.pl.ft) : dw_tile_kernel<float>(L.kernel, L.pl.ct, L.pl.ft);
        CAPE_LAUNCH(k, grid, block, 0, st, p);
    }
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

// the reduction: the slabs of an earlier dw_contract of the same launch, summed in a fixed order into the gradient blocks
int dw_reduce(const DwLaunch &L, hipStream_t st) {
    if (L.rvec) CAPE_LAUNCH(dw_reduce_vec_kernel, dim3((unsigned)L.rblocks), dim3(256), 0, st, L.rp);
    else CAPE_LAUNCH(dw_reduce_kernel, dim3((unsigned)L.rblocks), dim3(256), 0, st, L.rp);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

// the arguments of an entry point / an item of a batch as a DwCall (the bf16 entry points' void * become float * here)
inline DwCall dw_call(const cape_src_t *srcs, int32_t nsrc, const void *dz, int64_t dz_sample_stride, int32_t lddz, const void *dz2,
                      uint32_t dz2_mask, int32_t N, int32_t Mo, int32_t F, bool bf16, const cape_h2_dw_t *h2 = nullptr,
                      int32_t accumulate = 0, void *workspace = nullptr, int64_t workspace_bytes = 0) {
    return DwCall{srcs, nsrc, N, Mo, F, accumulate, (const float *)dz, (const float *)dz2, dz_sample_stride, lddz, dz2_mask,
                  workspace, workspace_bytes, bf16, h2};
}
inline DwCall dw_call(const cape_dw_item_t &t) {
    return dw_call(t.srcs, t.nsrc, t.dz, t.dz_sample_stride, t.lddz, t.dz2, t.dz2_mask, t.N, t.Mo, t.F, t.bf16 != 0, t.h2, t.accumulate,
                   t.workspace, t.workspace_bytes);
}

// plan[0..3] = kernel id, tile rows (channels), tile columns, partial slabs
int dw_plan_query(const DwCall &c, int32_t plan[4]) {
    if (!plan) return CAPE_EINVAL;
    DwLaunch L;
    const int rc = dw_resolve(c, L, false);
    if (rc) return rc;
    plan[0] = L.kernel; plan[1] = L.pl.ct; plan[2] = L.pl.ft; plan[3] = L.pl.ngroups * L.pl.rsplit;
    return CAPE_OK;
}

// stage 0: contraction and reduction, 1: contraction only, 2: reduction only (of an earlier stage-1 call with the same arguments)
int dw_run(const DwCall &c, int stage, void *stream) {
    if (stage < 0 || stage > 2) return CAPE_EINVAL;
    DwLaunch L;
    int rc = dw_resolve(c, L);
    if (rc == CAPE_OK && stage <= 1) rc = dw_contract(L, (hipStream_t)stream);
    if (rc == CAPE_OK && stage != 1) rc = dw_reduce(L, (hipStream_t)stream);
    return rc;
}
}  // namespace

extern "C" int cape_gconv_fwd_plan(const cape_src_t *srcs, int32_t nsrc, int32_t N, int32_t Mo, int32_t F, int32_t plan[4]) {
    return gconv_fwd_plan_impl(srcs, nsrc, N, Mo, F, plan, false);
}

extern "C" int cape_gconv_fwd_plan_bf16(const cape_src_t *srcs, int32_t nsrc, int32_t N, int32_t Mo, int32_t F, int32_t plan[4]) {
    return gconv_fwd_plan_impl(srcs, nsrc, N, Mo, F, plan, true);
}

extern "C" int cape_gconv_fwd(const cape_src_t *srcs, int32_t nsrc, float *y, int64_t y_sample_stride,
                              int32_t ldy, int32_t N, int32_t Mo, int32_t F, const float *bias,
                              int32_t bias_mode, int32_t act, uint32_t *mask_out, const cape_rank_t *rank,
                              int32_t out_deinterleave, void *stream) {
    return gconv_fwd_impl(srcs, nsrc, y, y_sample_stride, ldy, N, Mo, F, bias, bias_mode, act, mask_out, rank, out_deinterleave,
                          stream, false);
}

extern "C" int cape_gconv_fwd_h2(const cape_src_t *srcs, int32_t nsrc, float *y, int64_t y_sample_stride,
                                 int32_t ldy, int32_t N, int32_t Mo, int32_t F, const float *bias,
                                 int32_t bias_mode, int32_t act, uint32_t *mask_out, const cape_rank_t *rank,
                                 int32_t out_deinterleave, const cape_h2_t *h2, void *stream) {
    return gconv_fwd_impl(srcs, nsrc, y, y_sample_stride, ldy, N, Mo, F, bias, bias_mode, act, mask_out, rank, out_deinterleave,
                          stream, false, h2);
}

extern "C" int cape_gconv_fwd_plan_h2(const cape_src_t *srcs, int32_t nsrc, int32_t N, int32_t Mo, int32_t F, const cape_h2_t *h2,
                                      int32_t plan[4]) {
    return gconv_fwd_plan_impl(srcs, nsrc, N, Mo, F, plan, false, h2);
}

extern "C" int cape_gconv_fwd_bf16(const cape_src_t *srcs, int32_t nsrc, void *y, int64_t y_sample_stride,
                                   int32_t ldy, int32_t N, int32_t Mo, int32_t F, const float *bias,
                                   int32_t bias_mode, int32_t act, uint32_t *mask_out, const cape_rank_t *rank,
                                   int32_t out_deinterleave, void *stream) {
    return gconv_fwd_impl(srcs, nsrc, (float *)y, y_sample_stride, ldy, N, Mo, F, bias, bias_mode, act, mask_out, rank,
                          out_deinterleave, stream, true);
}

extern "C" int64_t cape_gconv_dw_workspace_bytes(const cape_src_t *srcs, int32_t nsrc, int32_t N,
                                                 int32_t Mo, int32_t F) {
    if (!srcs || nsrc < 1 || nsrc > CAPE_MAX_SRC || N < 1 || Mo < 1 || F < 1) return CAPE_EINVAL;
    // asked before dz (and with it the kernel) is known: the larger of the two tile plans a launch can end up with
    DwPlan pl;
    plan_dw(srcs, nsrc, N, Mo, F, pl);
    const long long generic = dw_workspace_need(pl);
    plan_dw_plain(srcs, nsrc, N, Mo, F, true, pl);
    return (int64_t)std::max(generic, dw_workspace_need(pl));
}

extern "C" int cape_gconv_dw_plan(const cape_src_t *srcs, int32_t nsrc, const float *dz, int64_t dz_sample_stride,
                                  int32_t lddz, const float *dz2, uint32_t dz2_mask, int32_t N, int32_t Mo, int32_t F,
                                  int32_t plan[4]) {
    return dw_plan_query(dw_call(srcs, nsrc, dz, dz_sample_stride, lddz, dz2, dz2_mask, N, Mo, F, false), plan);
}

extern "C" int cape_gconv_dw_plan_h2(const cape_src_t *srcs, int32_t nsrc, const float *dz, int64_t dz_sample_stride,
                                     int32_t lddz, const float *dz2, uint32_t dz2_mask, int32_t N, int32_t Mo, int32_t F,
                                     const cape_h2_dw_t *h2, int32_t plan[4]) {
    return dw_plan_query(dw_call(srcs, nsrc, dz, dz_sample_stride, lddz, dz2, dz2_mask, N, Mo, F, false, h2), plan);
}

extern "C" int cape_gconv_dw_plan_bf16(const cape_src_t *srcs, int32_t nsrc, const void *dz, int64_t dz_sample_stride,
                                       int32_t lddz, const void *dz2, uint32_t dz2_mask, int32_t N, int32_t Mo, int32_t F,
                                       int32_t plan[4]) {
    return dw_plan_query(dw_call(srcs, nsrc, dz, dz_sample_stride, lddz, dz2, dz2_mask, N, Mo, F, true), plan);
}

extern "C" int cape_gconv_dw_stage(const cape_src_t *srcs, int32_t nsrc, const float *dz,
                                   int64_t dz_sample_stride, int32_t lddz, const float *dz2, uint32_t dz2_mask,
                                   int32_t N, int32_t Mo, int32_t F, int32_t accumulate, void *workspace,
                                   int64_t workspace_bytes, int32_t stage, void *stream) {
    return dw_run(dw_call(srcs, nsrc, dz, dz_sample_stride, lddz, dz2, dz2_mask, N, Mo, F, false, nullptr, accumulate, workspace,
                          workspace_bytes), stage, stream);
}

extern "C" int cape_gconv_dw(const cape_src_t *srcs, int32_t nsrc, const float *dz,
                             int64_t dz_sample_stride, int32_t lddz, const float *dz2, uint32_t dz2_mask,
                             int32_t N, int32_t Mo, int32_t F, int32_t accumulate, void *workspace,
                             int64_t workspace_bytes, void *stream) {
    return cape_gconv_dw_stage(srcs, nsrc, dz, dz_sample_stride, lddz, dz2, dz2_mask, N, Mo, F, accumulate, workspace,
                               workspace_bytes, 0, stream);
}

extern "C" int cape_gconv_dw_stage_h2(const cape_src_t *srcs, int32_t nsrc, const float *dz,
                                      int64_t dz_sample_stride, int32_t lddz, const float *dz2, uint32_t dz2_mask,
                                      int32_t N, int32_t Mo, int32_t F, int32_t accumulate, void *workspace,
                                      int64_t workspace_bytes, int32_t stage, const cape_h2_dw_t *h2, void *stream) {
    return dw_run(dw_call(srcs, nsrc, dz, dz_sample_stride, lddz, dz2, dz2_mask, N, Mo, F, false, h2, accumulate, workspace,
                          workspace_bytes), stage, stream);
}

extern "C" int cape_gconv_dw_stage_bf16(const cape_src_t *srcs, int32_t nsrc, const void *dz,
                                        int64_t dz_sample_stride, int32_t lddz, const void *dz2, uint32_t dz2_mask,
                                        int32_t N, int32_t Mo, int32_t F, int32_t accumulate, void *workspace,
                                        int64_t workspace_bytes, int32_t stage, void *stream) {
    return dw_run(dw_call(srcs, nsrc, dz, dz_sample_stride, lddz, dz2, dz2_mask, N, Mo, F, true, nullptr, accumulate, workspace,
                          workspace_bytes), stage, stream);
}

extern "C" int cape_gconv_dw_bf16(const cape_src_t *srcs, int32_t nsrc, const void *dz,
                                  int64_t dz_sample_stride, int32_t lddz, const void *dz2, uint32_t dz2_mask,
                                  int32_t N, int32_t Mo, int32_t F, int32_t accumulate, void *workspace,
                                  int64_t workspace_bytes, void *stream) {
    return cape_gconv_dw_stage_bf16(srcs, nsrc, dz, dz_sample_stride, lddz, dz2, dz2_mask, N, Mo, F, accumulate, workspace,
                                    workspace_bytes, 0, stream);
}

// the slab reductions of several launches (each contracted before with the same arguments) as one grid
extern "C" int cape_gconv_dw_reduce_batch(const cape_dw_item_t *items, int32_t nitems, void *stream) {
    if (!items || nitems < 1 || nitems > CAPE_MAX_DW_REDUCE_ITEMS) return CAPE_EINVAL;
    DwReduceBatch B;
    B.n = nitems;
    int off = 0;
    for (int i = 0; i < nitems; ++i) {
        DwLaunch L;
        const int rc = dw_resolve(dw_call(items[i]), L);
        if (rc) return rc;
        B.it[i] = L.rp;
        B.vec[i] = L.rvec ? 1 : 0;
        B.blk_off[i] = off;
        off += L.rblocks;
    }
    B.blk_off[nitems] = off;
    CAPE_LAUNCH(dw_reduce_batch_kernel, dim3((unsigned)off), dim3(256), 0, (hipStream_t)stream, B);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

// =============================================================================================================
// Weight gradients per phase: the contractions of several queued launches of dw_h2_kernel<128, 128, true> as ONE grid
// (DwBatch, gconv_shared.h).  Every item keeps the contraction splits of its own launch -- the same partial slabs in the same
// workspace, so the reduction and the gradients are those of the per-layer launches bit for bit -- but the tiles of all items
// queue for the chip together: one launch's ramp and drain instead of one per layer, the longest workgroups first.  (Cutting
// the items into FEWER splits for the shared grid was built and measured too: 2.3-2.8 % of the step instead of 1.7 %, but
// fewer, longer partial sums move the gradients' rounding by 2e-6 of their maximum)  The plan is
// a pure function of the items' shapes.
// =============================================================================================================
namespace {
struct DwbShape { int N, tiles, nseg, ngroups, rsplit, rows_per_split; };     // the item's own plan
struct DwbLaunch {
    int first, n;                                                 // items first .. first + n - 1 of the list
    int order[DWB_MAX_ITEMS];                                     // table position -> item of the launch: longest workgroups first
    int rot[DWB_MAX_ITEMS];                                       // (by table position) XCD of split 0
    int start[8][DWB_MAX_ITEMS + 2];
    int grid, units;
};

// splits of an item (rotation rot) that run on XCD x: s = ((x - rot) & 7) + 8 q < count
inline int dwb_on_xcd(int count, int rot, int x) {
    const int s0 = (x - rot) & 7;
    return s0 < count ? (count - 1 - s0) / 8 + 1 : 0;
}

// One launch: the items' places on the 8 XCDs.
inline void dwb_plan_launch(const DwbShape *sh, int n, DwbLaunch &L) {
    long long rows[DWB_MAX_ITEMS];
    L.units = 0;
    for (int i = 0; i < n; ++i) {
        L.order[i] = i;
        rows[i] = (long long)(sh[i].N / sh[i].ngroups) * sh[i].rows_per_split;
        L.units += sh[i].tiles * sh[i].ngroups * sh[i].rsplit;
    }
    // table order: longest workgroups first (then list order); each item's rotation: the one that leaves the busiest XCD
    // with the least work (tiles x rows), the lowest on a tie
    std::stable_sort(L.order, L.order + n, [&](int a, int b) { return rows[a] > rows[b]; });
    long long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < n; ++k) {
        const int i = L.order[k], count = sh[i].ngroups * sh[i].rsplit;
        const long long w = (long long)sh[i].tiles * rows[i];
        int best = 0;
        long long best_peak = -1;
        for (int r = 0; r < 8; ++r) {
            long long peak = 0;
            for (int x = 0; x < 8; ++x) {
                const long long v = load[x] + w * dwb_on_xcd(count, r, x);
                peak = v > peak ? v : peak;
            }
            if (best_peak < 0 || peak < best_peak) { best_peak = peak; best = r; }
        }
        L.rot[k] = best;
        for (int x = 0; x < 8; ++x) load[x] += w * dwb_on_xcd(count, best, x);
    }
    int longest = 0;
    for (int x = 0; x < 8; ++x) {
        int start = 0;
        for (int k = 0; k < DWB_MAX_ITEMS + 2; ++k) {
            L.start[x][k] = start;
            if (k < n) start += sh[L.order[k]].tiles * dwb_on_xcd(sh[L.order[k]].ngroups * sh[L.order[k]].rsplit, L.rot[k], x);
        }
        longest = start > longest ? start : longest;
    }
    L.grid = 8 * longest;
}

// The list cut into launches (in list order: what the argument table holds), each planned on its own.
inline void dwb_plan(const DwbShape *sh, int n, std::vector<DwbLaunch> &out) {
    out.clear();
    int i = 0;
    while (i < n) {
        DwbLaunch L;
        L.first = i;
        int segs = 0, k = 0;
        while (i + k < n && k < DWB_MAX_ITEMS && segs + sh[i + k].nseg <= DWB_MAX_SEGS) {
            segs += sh[i + k].nseg;
            ++k;
        }
        L.n = k;
        dwb_plan_launch(sh + i, k, L);
        out.push_back(L);
        i += k;
    }
}

// an item of the list: does it run dw_h2_kernel<128, 128, true>, and with which tiles and splits?
inline int dwb_describe(const cape_dw_item_t &t, DwLaunch &d, DwbShape &s) {
    if (t.bf16 || !t.h2) return CAPE_EINVAL;
    const int rc = dw_resolve(dw_call(t), d);
    if (rc) return rc;
    if (d.kernel != DW_H2 || !d.v4 || t.nsrc > DWB_MAX_SEGS) return CAPE_EINVAL;
    s.N = t.N; s.nseg = t.nsrc;
    s.tiles = d.pl.ntiles;
    s.ngroups = d.pl.ngroups; s.rsplit = d.pl.rsplit; s.rows_per_split = d.pl.rows_per_split;
    return CAPE_OK;
}

int dwb_prepare(const cape_dw_item_t *items, int nitems, std::vector<DwLaunch> &desc, std::vector<DwbShape> &sh,
                std::vector<DwbLaunch> &launches) {
    if (!items || nitems < 1 || nitems > CAPE_MAX_DW_REDUCE_ITEMS) return CAPE_EINVAL;
    desc.resize(nitems);
    sh.resize(nitems);
    for (int i = 0; i < nitems; ++i) {
        const int rc = dwb_describe(items[i], desc[i], sh[i]);
        if (rc) return rc;
    }
    dwb_plan(sh.data(), nitems, launches);
    return CAPE_OK;
}
}  // namespace

extern "C" int cape_gconv_dw_batch_plan(const cape_dw_item_t *items, int32_t nitems, int32_t *units, int32_t max_units, int32_t info[4]) {
    std::vector<DwLaunch> desc;
    std::vector<DwbShape> sh;
    std::vector<DwbLaunch> launches;
    const int rc = dwb_prepare(items, nitems, desc, sh, launches);
    if (rc) return rc;
    if (!info) return CAPE_EINVAL;
    int nunits = 0, grid = 0;
    for (size_t l = 0; l < launches.size(); ++l) {
        const DwbLaunch &L = launches[l];
        grid = L.grid > grid ? L.grid : grid;
        // the workgroups as the kernel decodes them: XCD x, the items in table order, an item's splits on x, a split's tiles
        for (int x = 0; x < 8; ++x)
            for (int tk = 0; tk < L.n; ++tk) {
                const int k = L.order[tk];
                const DwLaunch &d = desc[L.first + k];
                const DwbShape &c = sh[L.first + k];
                const int spg = c.N / c.ngroups;
                for (int j = L.start[x][tk]; j < L.start[x][tk + 1]; ++j, ++nunits) {
                    if (!units || nunits >= max_units) continue;
                    const int q = (j - L.start[x][tk]) / c.tiles, t = (j - L.start[x][tk]) % c.tiles;
                    const int split = ((x - L.rot[tk]) & 7) + 8 * q;
                    int si = 0;
                    while (si + 1 < d.p.nsrc && t >= d.p.tile_off[si + 1]) ++si;
                    const int grp = split / c.rsplit, rs = split % c.rsplit;
                    const int wra = rs * c.rows_per_split, rb = wra + c.rows_per_split < d.p.Mo ? wra + c.rows_per_split : d.p.Mo;
                    int32_t *u = units + 10 * (size_t)nunits;
                    u[0] = (int32_t)l; u[1] = 8 * j + x; u[2] = L.first + k; u[3] = si; u[4] = t - d.p.tile_off[si];
                    u[5] = split; u[6] = grp * spg; u[7] = grp * spg + spg; u[8] = wra; u[9] = rb;
                }
            }
    }
    info[0] = (int32_t)launches.size(); info[1] = nunits; info[2] = (int32_t)sizeof(DwParams); info[3] = grid;
    return CAPE_OK;
}

extern "C" int cape_gconv_dw_batch(const cape_dw_item_t *items, int32_t nitems, void *stream) {
    std::vector<DwLaunch> desc;
    std::vector<DwbShape> sh;
    std::vector<DwbLaunch> launches;
    const int rc = dwb_prepare(items, nitems, desc, sh, launches);
    if (rc) return rc;
    for (const DwbLaunch &L : launches) {
        DwParams P = DwParams();
        DwBatch &B = P.bt;
        int seg = 0;
        for (int tk = 0; tk < L.n; ++tk) {                        // (table order)
            const int k = L.order[tk];
            const DwParams &p = desc[L.first + k].p;
            DwBatchItem &it = B.item[tk];
            it.dz = p.dz; it.dzrm = p.dzrm; it.dz2 = p.dz2; it.dz2rm = p.dz2rm; it.dzs = p.dzs;
            it.ws = p.ws; it.slab = p.slab;
            it.lddz = p.lddz; it.dzrmw = p.dzrmw; it.dz2rmw = p.dz2rmw; it.F = p.F; it.N = p.N; it.Mo = p.Mo; it.ftiles = p.ftiles;
            it.rsplit = p.rsplit; it.rows_per_split = p.rows_per_split; it.samples_per_group = p.samples_per_group;
            it.seg0 = seg; it.nseg = p.nsrc;
            it.ntiles = sh[L.first + k].tiles; it.rot = L.rot[tk];
            for (int s = 0; s < p.nsrc; ++s, ++seg) {
                DwBatchSeg &sg = B.seg[seg];
                sg.x = p.s[s].x; sg.rm = p.s[s].rm; sg.xs = p.s[s].xs; sg.part_off = p.part_off[s];
                sg.ldx = p.s[s].ldx; sg.C = p.s[s].C;
                sg.rmw_use2 = p.s[s].rmw | (int)((p.dz2_mask >> s) & 1u) << 16;
                sg.tile_off = p.tile_off[s];
            }
        }
        B.nseg = seg;
        for (int x = 0; x < 8; ++x)
            for (int g = 0; g < DWB_MAX_ITEMS + 2; ++g) B.start[x][g] = L.start[x][g];
        if (L.grid < 8) return CAPE_EINVAL;
        CAPE_LAUNCH((dw_h2_kernel<128, 128, true>), dim3((unsigned)L.grid), dim3(256 * H2_DW_KG), 0, (hipStream_t)stream, P);
        CAPE_LAUNCH_CHECK();
    }
    return CAPE_OK;
}
