// Bandwidth-bound companions of the fused gather-GEMM (gfx950): bias/activation and their
// gradients, column reductions, condition-channel fill and reduction, the rank-1 term sums and
// the backward preparation with its finalize stage.  (The sparse-operator kernels: sparse.hip.)
// All kernels read/write [N, M, ld] views with channels contiguous and use float4 accesses
// whenever the view is 16-byte aligned.
#include "common.h"
#include "views.h"

namespace {

// ---- bias + activation ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void bias_act_kernel(CView x, const float *bias, int bias_mode, int act,
                                                       View y, int N, int M, int C) {
    const long long total = (long long)N * M * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long nm = i / C;
        const int m = (int)(nm % M);
        const int n = (int)(nm / M);
        float v = x.p[(long long)n * x.ss + (long long)m * x.ld + c];
        if (bias_mode == CAPE_BIAS_CHANNEL) v += bias[c];
        else if (bias_mode == CAPE_BIAS_VERTEX) v += bias[(long long)m * C + c];
        y.p[(long long)n * y.ss + (long long)m * y.ld + c] = cape_act(v, act);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void act_bwd_kernel(CView dy, CView y, int act, View dz, int N, int M, int C) {
    const int W = VEC ? 4 : 1;
    const int cq = C / W;
    const long long total = (long long)N * M * cq;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % cq) * W;
        const long long nm = i / cq;
        const int m = (int)(nm % M);
        const int n = (int)(nm / M);
        if (VEC) {
            const float4 g = *reinterpret_cast<const float4 *>(dy.p + (long long)n * dy.ss + (long long)m * dy.ld + c);
            const float4 o = *reinterpret_cast<const float4 *>(y.p + (long long)n * y.ss + (long long)m * y.ld + c);
            float4 r;
            r.x = g.x * cape_act_grad_from_out(o.x, act);
            r.y = g.y * cape_act_grad_from_out(o.y, act);
            r.z = g.z * cape_act_grad_from_out(o.z, act);
            r.w = g.w * cape_act_grad_from_out(o.w, act);
            *reinterpret_cast<float4 *>(dz.p + (long long)n * dz.ss + (long long)m * dz.ld + c) = r;
        } else {
            const float g = dy.p[(long long)n * dy.ss + (long long)m * dy.ld + c];
            const float o = y.p[(long long)n * y.ss + (long long)m * y.ld + c];
            dz.p[(long long)n * dz.ss + (long long)m * dz.ld + c] = g * cape_act_grad_from_out(o, act);
        }
    }
}

__global__ __launch_bounds__(256) void mask_mul_kernel(CView dy, const unsigned *mask, View dz, int N, int M, int F) {
    const int words = (F + 31) / 32;
    const long long total = (long long)N * M * F;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int f = (int)(i % F);
        const long long nm = i / F;
        const int m = (int)(nm % M);
        const int n = (int)(nm / M);
        const unsigned w = mask[nm * words + (f >> 5)];
        const float g = dy.p[(long long)n * dy.ss + (long long)m * dy.ld + f];
        dz.p[(long long)n * dz.ss + (long long)m * dz.ld + f] = ((w >> (f & 31)) & 1u) ? g : 0.f;
    }
}

// ---- column sums -----------------------------------------------------------------------------
// stage 1: block b sums rows [b*RB, (b+1)*RB) of the flattened (n,m) row space -> part[b][c]
constexpr int COLSUM_RB = 128;

// aligned fast path (C % 4 == 0): thread = (float4 column, row lane); column groups of <= 256 floats
__global__ __launch_bounds__(256) void colsum_partial_vec_kernel(CView x, int N, int M, int C, float *part) {
    __shared__ float4 red[256];
    const long long R = (long long)N * M;
    const long long ra = (long long)blockIdx.x * COLSUM_RB;
    const long long rb = (ra + COLSUM_RB < R) ? ra + COLSUM_RB : R;
    for (int cbase = 0; cbase < C; cbase += 256) {
        const int cw = min(256, C - cbase);
        const int c4n = cw >> 2;
        const int lanes = 256 / c4n;               // row lanes
        const int q = threadIdx.x % c4n, rl = threadIdx.x / c4n;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rl < lanes)
            for (long long r = ra + rl; r < rb; r += lanes) {
                const long long n = r / M, m = r % M;
                const float4 v = *reinterpret_cast<const float4 *>(x.p + n * x.ss + m * x.ld + cbase + 4 * q);
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
        red[threadIdx.x] = s;
        __syncthreads();
        if (rl == 0) {
            for (int l = 1; l < lanes; ++l) {
                const float4 v = red[l * c4n + q];
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
            *reinterpret_cast<float4 *>(part + (long long)blockIdx.x * C + cbase + 4 * q) = s;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void colsum_partial_kernel(CView x, int N, int M, int C, float *part) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const long long R = (long long)N * M;
    const long long ra = (long long)blockIdx.x * COLSUM_RB;
    const long long rb = (ra + COLSUM_RB < R) ? ra + COLSUM_RB : R;
    for (int cbase = 0; cbase < C; cbase += 64) {
        const int c = cbase + cl;
        float s = 0.f;
        if (c < C)
            for (long long r = ra + rl; r < rb; r += 4) {
                const long long n = r / M, m = r % M;
                s += x.p[n * x.ss + m * x.ld + c];
            }
        red[rl][cl] = s;
        __syncthreads();
        if (rl == 0 && c < C) part[(long long)blockIdx.x * C + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
        __syncthreads();
    }
}

// stage 2: block = 64 columns x 4 partial lanes
__global__ __launch_bounds__(256) void colsum_final_kernel(const float *part, int nblk, int C, int accumulate, float *out) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, pl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    float s = 0.f;
    if (c < C)
        for (int b = pl; b < nblk; b += 4) s += part[(long long)b * C + c];
    red[pl][cl] = s;
    __syncthreads();
    if (pl == 0 && c < C) {
        const float t = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
        out[c] = accumulate ? out[c] + t : t;
    }
}

template <typename T = float>
__global__ __launch_bounds__(256) void sum_over_samples_kernel(CViewT<T> x, int N, int M, int C, int accumulate, float *out) {
    const long long total = (long long)M * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long m = i / C;
        float s = 0.f;
        for (int n = 0; n < N; ++n) s += cape_ld(x.p + (long long)n * x.ss + m * x.ld + c);
        out[i] = accumulate ? out[i] + s : s;
    }
}

// ---- condition channels ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void fill_cond_kernel(const float *cond, int ldc, const float *scale, View y,
                                                        int N, int M, int C) {
    const long long total = (long long)N * M * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const long long nm = i / C;
        const int m = (int)(nm % M);
        const int n = (int)(nm / M);
        float v = cond[(long long)n * ldc + c];
        if (scale) v *= scale[m];
        y.p[(long long)n * y.ss + (long long)m * y.ld + c] = v;
    }
}

// dcond[n,c] (+)= sum_m scale[m] * dy[n,m,c]; one block per (n, 64-channel group)
__global__ __launch_bounds__(256) void reduce_cond_kernel(CView dy, const float *scale, float *dcond, int ldc,
                                                          int N, int M, int C, int accumulate) {
    __shared__ float red[4][64];
    const int cgroups = (C + 63) / 64;
    const int n = blockIdx.x / cgroups, cg = blockIdx.x % cgroups;
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = cg * 64 + cl;
    float s = 0.f;
    if (c < C)
        for (int m = rl; m < M; m += 4) {
            const float v = dy.p[(long long)n * dy.ss + (long long)m * dy.ld + c];
            s = scale ? fmaf(scale[m], v, s) : s + v;
        }
    red[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < C) {
        const float t = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
        float *d = dcond + (long long)n * ldc + c;
        *d = accumulate ? *d + t : t;
    }
}

// float4 form: thread = (channel quad, row lane), 256 / quads row lanes, two independent partial sums per lane --
// the scalar form above walks all M rows with four row lanes per block (208 us at M = 6890 for 32 condition channels)
__global__ __launch_bounds__(256) void reduce_cond_vec_kernel(CView dy, const float *scale, float *dcond, int ldc,
                                                              int N, int M, int C, int accumulate) {
    __shared__ float4 red[256];
    const int cgroups = (C + 63) / 64;
    const int n = blockIdx.x / cgroups, cg = blockIdx.x % cgroups;
    const int gw = min(64, C - cg * 64);                // channels of this block's group (C % 4 == 0)
    int qp = 1;
    while (qp < gw / 4) qp <<= 1;                       // quad lanes per row (power of two)
    const int RL = 256 / qp;
    const int q = threadIdx.x % qp, rl = threadIdx.x / qp;
    const int c = cg * 64 + 4 * q;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (4 * q < gw && c < C) {
        const float *p = dy.p + (long long)n * dy.ss + c;
        int m = rl;
        for (; m + RL < M; m += 2 * RL) {
            const float4 v0 = *reinterpret_cast<const float4 *>(p + (long long)m * dy.ld);
            const float4 v1 = *reinterpret_cast<const float4 *>(p + (long long)(m + RL) * dy.ld);
            const float s0 = scale ? scale[m] : 1.f, s1 = scale ? scale[m + RL] : 1.f;
            a.x = fmaf(s0, v0.x, a.x); a.y = fmaf(s0, v0.y, a.y); a.z = fmaf(s0, v0.z, a.z); a.w = fmaf(s0, v0.w, a.w);
            b.x = fmaf(s1, v1.x, b.x); b.y = fmaf(s1, v1.y, b.y); b.z = fmaf(s1, v1.z, b.z); b.w = fmaf(s1, v1.w, b.w);
        }
        if (m < M) {
            const float4 v0 = *reinterpret_cast<const float4 *>(p + (long long)m * dy.ld);
            const float s0 = scale ? scale[m] : 1.f;
            a.x = fmaf(s0, v0.x, a.x); a.y = fmaf(s0, v0.y, a.y); a.z = fmaf(s0, v0.z, a.z); a.w = fmaf(s0, v0.w, a.w);
        }
    }
    red[threadIdx.x] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
    __syncthreads();
    if (threadIdx.x < qp && 4 * threadIdx.x < gw && cg * 64 + 4 * (int)threadIdx.x < C) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int l = 0; l < RL; ++l) {
            const float4 v = red[l * qp + threadIdx.x];
            t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
        }
        float *d = dcond + (long long)n * ldc + cg * 64 + 4 * threadIdx.x;
        if (accumulate) { t.x += d[0]; t.y += d[1]; t.z += d[2]; t.w += d[3]; }
        d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
    }
}

// ---- out[n, j, f] = sum_r rowscale[j, r] * dz[n, r, f]   (gradient of the rank-1 condition terms)
constexpr int RSR_RB = 32;    // rows per block
constexpr int RSR_MAXR = 4;

// stage 1: block = (sample n, row chunk), thread = (column, row lane); part[n][chunk][j][f]
__global__ __launch_bounds__(256) void rowscale_partial_kernel(CView dz, const float *rowscale, int R, int N, int Mo, int F,
                                                               float *part, int chunks) {
    __shared__ float red[RSR_MAXR][256];
    const int n = blockIdx.x / chunks, ch = blockIdx.x % chunks;
    const int ra = ch * RSR_RB, rb = min(Mo, ra + RSR_RB);
    for (int fbase = 0; fbase < F; fbase += 64) {
        const int fl = threadIdx.x & 63, rl = threadIdx.x >> 6;
        const int f = fbase + fl;
        float acc[RSR_MAXR] = {0.f, 0.f, 0.f, 0.f};
        if (f < F)
            for (int r = ra + rl; r < rb; r += 4) {
                const float v = dz.p[(long long)n * dz.ss + (long long)r * dz.ld + f];
#pragma unroll
                for (int j = 0; j < RSR_MAXR; ++j)
                    if (j < R) acc[j] = fmaf(rowscale[(long long)j * Mo + r], v, acc[j]);
            }
#pragma unroll
        for (int j = 0; j < RSR_MAXR; ++j) red[j][threadIdx.x] = acc[j];
        __syncthreads();
        if (rl == 0 && f < F) {
#pragma unroll
            for (int j = 0; j < RSR_MAXR; ++j)
                if (j < R)
                    part[(((long long)n * chunks + ch) * R + j) * F + f] =
                        (red[j][fl] + red[j][64 + fl]) + (red[j][128 + fl] + red[j][192 + fl]);
        }
        __syncthreads();
    }
}

// stage 2: out[n][j][f] = sum_chunk part[n][chunk][j][f]; block = 64 (j,f) elements x 4 chunk lanes
__global__ __launch_bounds__(256) void rowscale_final_kernel(const float *part, int chunks, int RF, int N, float *out) {
    __shared__ float red[4][64];
    const int el = threadIdx.x & 63, cl = threadIdx.x >> 6;
    const int blocks_per_n = (RF + 63) / 64;
    const int n = blockIdx.x / blocks_per_n;
    const int e = (blockIdx.x % blocks_per_n) * 64 + el;
    float s = 0.f;
    if (e < RF)
        for (int c = cl; c < chunks; c += 4) s += part[((long long)n * chunks + c) * RF + e];
    red[cl][el] = s;
    __syncthreads();
    if (cl == 0 && e < RF) out[(long long)n * RF + e] = (red[0][el] + red[1][el]) + (red[2][el] + red[3][el]);
}

// ---- fused backward preparation: dz, bias gradient and rank-1 term gradients in one pass over g ----
constexpr int BP_RB_MAX = 128;              // rows per block (upper bound; halved until the grid has BP_BLOCKS blocks)
#ifndef CAPE_BP_BLOCKS_DEFAULT
#define CAPE_BP_BLOCKS_DEFAULT 448
#endif
#ifndef CAPE_BP_UNROLL_DEFAULT
#define CAPE_BP_UNROLL_DEFAULT 2           // rows loaded ahead per thread in bwd_prep_vec_kernel (compile-time: 1, 2, 4)
#endif
#ifndef CAPE_BP_RB_MIN_DEFAULT
#define CAPE_BP_RB_MIN_DEFAULT 16
#endif
inline int bp_rows(int N, int Mo) {
    constexpr int want = CAPE_BP_BLOCKS_DEFAULT, rbmin = CAPE_BP_RB_MIN_DEFAULT;      // (measured in round 2; no run-time knob)
    int rb = BP_RB_MAX;
    while (rb > rbmin && (long long)N * ((Mo + rb - 1) / rb) < want) rb >>= 1;
    return rb;
}
constexpr int BP_MAXT = RSR_MAXR + 2;       // reduction terms: [0]=sum dz, [1..R]=rowscale_j*dz, [R+1]=rowscale_rg*g

template <typename AT = float>
__global__ __launch_bounds__(256) void bwd_prep_kernel(CViewT<AT> g, CViewT<AT> y, int act, const unsigned *mask, ViewT<AT> dz,
                                                       const float *rowscale, int R, int rg, int want_bias, int want_g,
                                                       int N, int Mo, int F, float *part, int chunks, int RB) {
    __shared__ float red[BP_MAXT][256];
    const int n = blockIdx.x / chunks, ch = blockIdx.x % chunks;
    const int ra = ch * RB, rb = min(Mo, ra + RB);
    const int words = (F + 31) / 32;
    const int T = R + 2;
    const int fl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    for (int fbase = 0; fbase < F; fbase += 64) {
        const int f = fbase + fl;
        float acc[BP_MAXT];
#pragma unroll
        for (int j = 0; j < BP_MAXT; ++j) acc[j] = 0.f;
        if (f < F)
            for (int r = ra + rl; r < rb; r += 4) {
                const float gv = cape_ld(g.p + (long long)n * g.ss + (long long)r * g.ld + f);
                float d;
                if (mask) d = ((mask[((long long)n * Mo + r) * words + (f >> 5)] >> (f & 31)) & 1u) ? gv : 0.f;
                else if (act != CAPE_ACT_NONE) d = gv * cape_act_grad_from_out(cape_ld(y.p + (long long)n * y.ss + (long long)r * y.ld + f), act);
                else d = gv;
                if (!((const void *)dz.p == (const void *)g.p && act == CAPE_ACT_NONE && !mask)) cape_st(dz.p + (long long)n * dz.ss + (long long)r * dz.ld + f, d);
                acc[0] += d;
#pragma unroll
                for (int j = 0; j < RSR_MAXR; ++j)
                    if (j < R) acc[1 + j] = fmaf(rowscale[(long long)j * Mo + r], d, acc[1 + j]);
                if (want_g) acc[BP_MAXT - 1] = fmaf(rowscale[(long long)rg * Mo + r], gv, acc[BP_MAXT - 1]);
            }
#pragma unroll
        for (int j = 0; j < BP_MAXT; ++j) red[j][threadIdx.x] = acc[j];
        __syncthreads();
        if (rl == 0 && f < F) {
            float *pp = part + ((long long)n * chunks + ch) * T * F;
            if (want_bias) pp[f] = (red[0][fl] + red[0][64 + fl]) + (red[0][128 + fl] + red[0][192 + fl]);
#pragma unroll
            for (int j = 0; j < RSR_MAXR; ++j)
                if (j < R) pp[(1 + j) * F + f] = (red[1 + j][fl] + red[1 + j][64 + fl]) + (red[1 + j][128 + fl] + red[1 + j][192 + fl]);
            if (want_g) pp[(R + 1) * F + f] = (red[BP_MAXT - 1][fl] + red[BP_MAXT - 1][64 + fl]) +
                                              (red[BP_MAXT - 1][128 + fl] + red[BP_MAXT - 1][192 + fl]);
        }
        __syncthreads();
    }
}

// narrow variant (F <= 4: the 3-channel output layer): thread = ROW, its F columns in registers.  The column-lane mapping
// above keeps 3 of 64 lanes busy there, each walking its rows one dependent access at a time (24 us for 2 MB).
template <typename AT = float>
__global__ __launch_bounds__(256) void bwd_prep_narrow_kernel(CViewT<AT> g, CViewT<AT> y, int act, const unsigned *mask, ViewT<AT> dz,
                                                              const float *rowscale, int R, int rg, int want_bias, int want_g,
                                                              int N, int Mo, int F, float *part, int chunks, int RB) {
    __shared__ float red[4][BP_MAXT * 4];
    const int n = blockIdx.x / chunks, ch = blockIdx.x % chunks;
    const int ra = ch * RB, rb = min(Mo, ra + RB);
    const int T = R + 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float acc[BP_MAXT][4];
#pragma unroll
    for (int j = 0; j < BP_MAXT; ++j)
#pragma unroll
        for (int f = 0; f < 4; ++f) acc[j][f] = 0.f;
    for (int r = ra + (int)threadIdx.x; r < rb; r += 256) {
        float gv[4], rs[RSR_MAXR], rsg = 0.f;
        const unsigned mw = mask ? mask[(long long)n * Mo + r] : 0u;            // F <= 4: one sign word per row
#pragma unroll
        for (int f = 0; f < 4; ++f) gv[f] = f < F ? cape_ld(g.p + (long long)n * g.ss + (long long)r * g.ld + f) : 0.f;
#pragma unroll
        for (int j = 0; j < RSR_MAXR; ++j) rs[j] = j < R ? rowscale[(long long)j * Mo + r] : 0.f;
        if (want_g) rsg = rowscale[(long long)rg * Mo + r];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            if (f >= F) continue;
            float d;
            if (mask) d = ((mw >> f) & 1u) ? gv[f] : 0.f;
            else if (act != CAPE_ACT_NONE) d = gv[f] * cape_act_grad_from_out(cape_ld(y.p + (long long)n * y.ss + (long long)r * y.ld + f), act);
            else d = gv[f];
            if (!((const void *)dz.p == (const void *)g.p && act == CAPE_ACT_NONE && !mask)) cape_st(dz.p + (long long)n * dz.ss + (long long)r * dz.ld + f, d);
            acc[0][f] += d;
#pragma unroll
            for (int j = 0; j < RSR_MAXR; ++j) acc[1 + j][f] = fmaf(rs[j], d, acc[1 + j][f]);
            acc[BP_MAXT - 1][f] = fmaf(rsg, gv[f], acc[BP_MAXT - 1][f]);
        }
    }
    // fixed-order sums: the lanes of a wave (xor butterflies), then the four waves
#pragma unroll
    for (int j = 0; j < BP_MAXT; ++j)
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            float v = acc[j][f];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
            if (lane == 0) red[wave][j * 4 + f] = v;
        }
    __syncthreads();
    if (threadIdx.x < BP_MAXT * 4) {
        const int j = threadIdx.x >> 2, f = threadIdx.x & 3;
        const float t = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
        float *pp = part + ((long long)n * chunks + ch) * T * F;
        if (f < F) {
            if (j == 0) { if (want_bias) pp[f] = t; }
            else if (j == BP_MAXT - 1) { if (want_g) pp[(R + 1) * F + f] = t; }
            else if (j - 1 < R) pp[j * F + f] = t;
        }
    }
}

// vector variant (F % VW == 0, aligned views): thread = (column group of VW channels, row lane).  The rows of a lane are
// taken UR at a time: the UR gradient rows (and their sign words / outputs) are all loaded before the first is used, so a
// thread waits for one memory round trip per UR rows instead of one per row.
template <typename AT, int VW, int UR>
__global__ __launch_bounds__(256) void bwd_prep_vec_kernel(CViewT<AT> g, CViewT<AT> y, int act, const unsigned *mask, ViewT<AT> dz,
                                                           const float *rowscale, int R, int rg, int want_bias, int want_g,
                                                           int N, int Mo, int F, float *part, int chunks, int RB, float *rm) {
    __shared__ float red[VW][256];
    const int n = blockIdx.x / chunks, ch = blockIdx.x % chunks;
    const int ra = ch * RB, rb = min(Mo, ra + RB);
    const int words = (F + 31) / 32;
    const int T = R + 2;
    constexpr int FB = 64 * VW;                 // channels per column pass (256 threads x VW >= FB)
    float *pp = part + ((long long)n * chunks + ch) * T * F;
    const AT *gb = g.p + (long long)n * g.ss;
    const AT *yb = y.p ? y.p + (long long)n * y.ss : nullptr;
    AT *zb = dz.p + (long long)n * dz.ss;
    const bool wr = !((const void *)dz.p == (const void *)g.p && act == CAPE_ACT_NONE && !mask);      // dz == g unchanged: the caller wants the sums only
    const unsigned *mb = mask ? mask + (long long)n * Mo * words : nullptr;
    for (int fbase = 0; fbase < F; fbase += FB) {
        const int fw = min(FB, F - fbase);
        const int cvn = fw / VW;                // column groups of this pass (divides 256)
        const int lanes = 256 / cvn;
        const int q = threadIdx.x % cvn, rl = threadIdx.x / cvn;
        const int f = fbase + VW * q;
        float acc[BP_MAXT][VW];
#pragma unroll
        for (int j = 0; j < BP_MAXT; ++j)
#pragma unroll
            for (int u = 0; u < VW; ++u) acc[j][u] = 0.f;
        for (int r0 = ra + rl; r0 < rb; r0 += UR * lanes) {
            float gv[UR][VW], ov[UR][VW];
            unsigned mw[UR];
#pragma unroll
            for (int k = 0; k < UR; ++k) {
                const int r = r0 + k * lanes;
                const int rr = r < rb ? r : r0;             // rows past the chunk re-read the first (result unused)
                cape_ldv<VW>(gb + (long long)rr * g.ld + f, gv[k]);
                if (mb) mw[k] = mb[(long long)rr * words + (f >> 5)] >> (f & 31);
                else if (act != CAPE_ACT_NONE) cape_ldv<VW>(yb + (long long)rr * y.ld + f, ov[k]);
            }
#pragma unroll
            for (int k = 0; k < UR; ++k) {
                const int r = r0 + k * lanes;
                if (r < rb) {
                    float d[VW];
#pragma unroll
                    for (int u = 0; u < VW; ++u) {
                        if (mb) d[u] = ((mw[k] >> u) & 1u) ? gv[k][u] : 0.f;
                        else if (act != CAPE_ACT_NONE) d[u] = gv[k][u] * cape_act_grad_from_out(ov[k][u], act);
                        else d[u] = gv[k][u];
                    }
                    if (wr) cape_stv<VW>(zb + (long long)r * dz.ld + f, d);
                    if (rm) {
                        // row bound of g -- and therefore of dz (|dz| <= |g| element by element): the affine block's backward
                        // contracts BOTH, one reduction serves the two.  Entry = column pass (F <= 4 * FB); the cvn lanes of a row
                        // are consecutive and aligned
                        float m = 0.f;
#pragma unroll
                        for (int u = 0; u < VW; ++u) m = fmaxf(m, fabsf(gv[k][u]));
                        m = cape_group_max(m, cvn);
                        if (q == 0) {
                            // (each pass writes only its own entry -- different threads own a row in different passes --
                            // and pass 0 zeroes the entries no pass owns)
                            float *dst = rm + 4 * ((long long)n * Mo + r);
                            dst[fbase / FB] = m;
                            if (fbase == 0)
                                for (int e = (F + FB - 1) / FB; e < 4; ++e) dst[e] = 0.f;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < VW; ++u) acc[0][u] += d[u];
#pragma unroll
                    for (int j = 0; j < RSR_MAXR; ++j)
                        if (j < R) {
                            const float sv = rowscale[(long long)j * Mo + r];
#pragma unroll
                            for (int u = 0; u < VW; ++u) acc[1 + j][u] = fmaf(sv, d[u], acc[1 + j][u]);
                        }
                    if (want_g) {
                        const float sv = rowscale[(long long)rg * Mo + r];
#pragma unroll
                        for (int u = 0; u < VW; ++u) acc[BP_MAXT - 1][u] = fmaf(sv, gv[k][u], acc[BP_MAXT - 1][u]);
                    }
                }
            }
        }
        // reduce the row lanes term by term: first inside each wave (the lanes of one column group are cvn apart: xor
        // shuffles over cvn, 2 cvn, ... 32), then the <= 4 per-wave (or per-lane, cvn >= 64) sums through LDS
        const int le = cvn < 64 ? 4 : lanes;                   // partial sums per column group that reach LDS
        const bool writer = cvn < 64 ? (int)(threadIdx.x & 63) < cvn : true;
        const int slot = cvn < 64 ? (int)(threadIdx.x >> 6) * cvn + q : (int)threadIdx.x;
#pragma unroll
        for (int j = 0; j < BP_MAXT; ++j) {
            const bool used = (j == 0 && want_bias) || (j >= 1 && j <= R) || (j == BP_MAXT - 1 && want_g);
            if (!used) continue;
            float v[VW];
#pragma unroll
            for (int u = 0; u < VW; ++u) v[u] = acc[j][u];
            for (int sh = cvn; sh < 64; sh <<= 1)
#pragma unroll
                for (int u = 0; u < VW; ++u) v[u] += __shfl_xor(v[u], sh);
            if (writer)
#pragma unroll
                for (int u = 0; u < VW; ++u) red[u][slot] = v[u];
            __syncthreads();
            if ((int)threadIdx.x < cvn) {
                float t[VW];
#pragma unroll
                for (int u = 0; u < VW; ++u) t[u] = red[u][q];
                for (int l = 1; l < le; ++l)
#pragma unroll
                    for (int u = 0; u < VW; ++u) t[u] += red[u][l * cvn + q];
                const int trow = (j == BP_MAXT - 1) ? (R + 1) : j;
                cape_stv<VW>(pp + (long long)trow * F + f, t);
            }
            __syncthreads();
        }
    }
}

// stage 2: block = (term t, 16 columns) x 16 lanes.  t = 0: dbias[f] = sum over (n, chunk);
// t = 1..R: dcoef[n, t-1, f] = sum over chunks; t = R+1: dcoef_g[n, f] = sum over chunks.
__device__ __forceinline__ void bwd_prep_final_block(int bid, const float *part, int chunks, int N, int F, int R, float *dbias,
                                                     float *dcoef, float *dcoef_g, long long cs, long long cgs) {
    __shared__ float red[16][17];
    const int T = R + 2;
    const int fblocks = (F + 15) / 16;
    const int fl = threadIdx.x & 15, ln = threadIdx.x >> 4;
    int b = bid;
    const int fb = b % fblocks; b /= fblocks;
    const int f = fb * 16 + fl;
    // block order: [bias blocks: fblocks] then for each n: (R+1) * fblocks
    float s = 0.f;
    float *dst = nullptr;
    if (b == 0) {            // bias
        if (dbias && f < F) {
            // sixteen independent partial sums: the chain of dependent L2 loads, not bandwidth, bounds this loop (the fused
            // activation-gradient form leaves one partial per spmm_multi workgroup: 16 x 216 per column in the benchmarked model,
            // 54 round trips with four sums)
            const long long total = (long long)N * chunks;
            const long long TF = (long long)T * F;
            constexpr int NS = 16;
            float ps[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) ps[k] = 0.f;
            long long i = ln;
            for (; i + 16 * (NS - 1) < total; i += 16 * NS) {
#pragma unroll
                for (int k = 0; k < NS; ++k) ps[k] += part[(i + 16 * k) * TF + f];
            }
            for (; i < total; i += 16) s += part[i * TF + f];
#pragma unroll
            for (int k = 0; k < NS; k += 4) s += (ps[k] + ps[k + 1]) + (ps[k + 2] + ps[k + 3]);
            dst = dbias + f;
        }
    } else {
        const int idx = b - 1;
        const int n = idx / (R + 1), t = 1 + idx % (R + 1);
        float *out = (t <= R) ? (dcoef ? dcoef + (long long)n * cs + (long long)(t - 1) * F : nullptr)
                              : (dcoef_g ? dcoef_g + (long long)n * cgs : nullptr);
        if (out && f < F) {
            for (int c = ln; c < chunks; c += 16) s += part[(((long long)n * chunks + c) * T + t) * F + f];
            dst = out + f;
        }
    }
    red[ln][fl] = s;
    __syncthreads();
    if (ln == 0 && dst) {
        float t = 0.f;
#pragma unroll
        for (int l = 0; l < 16; ++l) t += red[l][fl];
        *dst = t;
    }
}

__global__ __launch_bounds__(256) void bwd_prep_final_kernel(const float *part, int chunks, int N, int F, int R, float *dbias,
                                                             float *dcoef, float *dcoef_g, long long cs, long long cgs) {
    bwd_prep_final_block(blockIdx.x, part, chunks, N, F, R, dbias, dcoef, dcoef_g, cs, cgs);
}

// the final stage of SEVERAL bwd_prep calls in one launch (their partial slabs stay in their workspaces until then):
// the per-layer finals are 5 us dispatches whose results are only needed at the end of the backward pass
struct BpFinalBatch {
    struct I {
        const float *part;
        int chunks, N, F, R;
        float *dbias, *dcoef, *dcoef_g;
        long long cs, cgs;
    } it[CAPE_MAX_BWD_PREP_ITEMS];
    int blk_off[CAPE_MAX_BWD_PREP_ITEMS + 1];
    int n;
};

__global__ __launch_bounds__(256) void bwd_prep_final_batch_kernel(BpFinalBatch B) {
    int i = 0;
    while (i + 1 < B.n && (int)blockIdx.x >= B.blk_off[i + 1]) ++i;
    const BpFinalBatch::I &I = B.it[i];
    bwd_prep_final_block((int)blockIdx.x - B.blk_off[i], I.part, I.chunks, I.N, I.F, I.R, I.dbias, I.dcoef, I.dcoef_g, I.cs, I.cgs);
}

inline int grid_for(long long total) {
    long long b = (total + 255) / 256;
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace

extern "C" int cape_bias_act_fwd(const float *x, int64_t x_sample_stride, int32_t ldx, const float *bias,
                                 int32_t bias_mode, int32_t act, float *y, int64_t y_sample_stride, int32_t ldy,
                                 int32_t N, int32_t M, int32_t C, void *stream) {
    if (!x || !y || N < 1 || M < 1 || C < 1 || ldx < C || ldy < C) return CAPE_EINVAL;
    if (bias_mode != CAPE_BIAS_NONE && !bias) return CAPE_EINVAL;
    if (act < CAPE_ACT_NONE || act > CAPE_ACT_TANH) return CAPE_EINVAL;
    CView xv{x, x_sample_stride, ldx};
    View yv{y, y_sample_stride, ldy};
    CAPE_LAUNCH(bias_act_kernel, dim3(grid_for((long long)N * M * C)), dim3(256), 0, (hipStream_t)stream, xv, bias,
                       bias_mode, act, yv, N, M, C);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

extern "C" int cape_act_bwd(const float *dy, int64_t dy_sample_stride, int32_t lddy, const float *y,
                            int64_t y_sample_stride, int32_t ldy, int32_t act, float *dz, int64_t dz_sample_stride,
                            int32_t lddz, int32_t N, int32_t M, int32_t C, void *stream) {
    if (!dy || !y || !dz || N < 1 || M < 1 || C < 1 || lddy < C || ldy < C || lddz < C) return CAPE_EINVAL;
    if (act < CAPE_ACT_NONE || act > CAPE_ACT_TANH) return CAPE_EINVAL;
    CView gv{dy, dy_sample_stride, lddy}, ov{y, y_sample_stride, ldy};
    View zv{dz, dz_sample_stride, lddz};
    const bool vec = aligned4(dy, dy_sample_stride, lddy, C) && aligned4(y, y_sample_stride, ldy, C) &&
                     aligned4(dz, dz_sample_stride, lddz, C);
    hipStream_t st = (hipStream_t)stream;
    if (vec) CAPE_LAUNCH(act_bwd_kernel<true>, dim3(grid_for((long long)N * M * (C / 4))), dim3(256), 0, st, gv, ov, act, zv, N, M, C);
    else CAPE_LAUNCH(act_bwd_kernel<false>, dim3(grid_for((long long)N * M * C)), dim3(256), 0, st, gv, ov, act, zv, N, M, C);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

extern "C" int64_t cape_colsum_workspace_bytes(int32_t N, int32_t M, int32_t C) {
    if (N < 1 || M < 1 || C < 1) return CAPE_EINVAL;
    const long long R = (long long)N * M;
    const long long nblk = (R + COLSUM_RB - 1) / COLSUM_RB;
    return nblk * C * (int64_t)sizeof(float);
}

extern "C" int cape_colsum(const float *x, int64_t x_sample_stride, int32_t ldx, int32_t N, int32_t M, int32_t C,
                           int32_t per_vertex, int32_t accumulate, float *out, void *workspace,
                           int64_t workspace_bytes, void *stream) {
    if (!x || !out || N < 1 || M < 1 || C < 1 || ldx < C) return CAPE_EINVAL;
    CView xv{x, x_sample_stride, ldx};
    hipStream_t st = (hipStream_t)stream;
    if (per_vertex) {
        CAPE_LAUNCH((sum_over_samples_kernel<float>), dim3(grid_for((long long)M * C)), dim3(256), 0, st, xv, N, M, C, accumulate, out);
        CAPE_LAUNCH_CHECK();
        return CAPE_OK;
    }
    const long long R = (long long)N * M;
    const int nblk = (int)((R + COLSUM_RB - 1) / COLSUM_RB);
    if (!workspace || workspace_bytes < (int64_t)nblk * C * (int64_t)sizeof(float)) return CAPE_EWORKSPACE;
    if (aligned4(x, x_sample_stride, ldx, C) && (C >= 256 ? (C % 256) == 0 : (256 % (C / 4)) == 0))
        CAPE_LAUNCH(colsum_partial_vec_kernel, dim3(nblk), dim3(256), 0, st, xv, N, M, C, (float *)workspace);
    else
        CAPE_LAUNCH(colsum_partial_kernel, dim3(nblk), dim3(256), 0, st, xv, N, M, C, (float *)workspace);
    CAPE_LAUNCH_CHECK();
    CAPE_LAUNCH(colsum_final_kernel, dim3((C + 63) / 64), dim3(256), 0, st, (const float *)workspace, nblk, C, accumulate, out);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

/* per-vertex column sums of a bf16 tensor: out[m, c] (+)= sum_n x[n, m, c]  (gradient of the [1, M, F] output bias) */
extern "C" int cape_colsum_vertex_bf16(const void *x, int64_t x_sample_stride, int32_t ldx, int32_t N, int32_t M, int32_t C,
                                       int32_t accumulate, float *out, void *stream) {
    if (!x || !out || N < 1 || M < 1 || C < 1 || ldx < C) return CAPE_EINVAL;
    CViewT<cape_bf16> xv{(const cape_bf16 *)x, x_sample_stride, ldx};
    CAPE_LAUNCH((sum_over_samples_kernel<cape_bf16>), dim3(grid_for((long long)M * C)), dim3(256), 0, (hipStream_t)stream, xv, N, M, C,
                accumulate, out);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

extern "C" int cape_mask_mul(const float *dy, int64_t dy_sample_stride, int32_t lddy, const uint32_t *mask, float *dz,
                             int64_t dz_sample_stride, int32_t lddz, int32_t N, int32_t M, int32_t F, void *stream) {
    if (!dy || !mask || !dz || N < 1 || M < 1 || F < 1 || lddy < F || lddz < F) return CAPE_EINVAL;
    CView gv{dy, dy_sample_stride, lddy};
    View zv{dz, dz_sample_stride, lddz};
    CAPE_LAUNCH(mask_mul_kernel, dim3(grid_for((long long)N * M * F)), dim3(256), 0, (hipStream_t)stream, gv, mask, zv, N, M, F);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

extern "C" int cape_fill_cond(const float *cond, int32_t ldc, const float *scale, float *y, int64_t y_sample_stride,
                              int32_t ldy, int32_t N, int32_t M, int32_t C, void *stream) {
    if (!cond || !y || N < 1 || M < 1 || C < 1 || ldc < C || ldy < C) return CAPE_EINVAL;
    View yv{y, y_sample_stride, ldy};
    CAPE_LAUNCH(fill_cond_kernel, dim3(grid_for((long long)N * M * C)), dim3(256), 0, (hipStream_t)stream, cond, ldc, scale, yv, N, M, C);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

extern "C" int cape_reduce_cond(const float *dy, int64_t dy_sample_stride, int32_t lddy, const float *scale, float *dcond,
                                int32_t ldc, int32_t N, int32_t M, int32_t C, int32_t accumulate, void *stream) {
    if (!dy || !dcond || N < 1 || M < 1 || C < 1 || lddy < C || ldc < C) return CAPE_EINVAL;
    CView gv{dy, dy_sample_stride, lddy};
    const int cgroups = (C + 63) / 64;
    if (aligned4(dy, dy_sample_stride, lddy, C))
        CAPE_LAUNCH(reduce_cond_vec_kernel, dim3(N * cgroups), dim3(256), 0, (hipStream_t)stream, gv, scale, dcond, ldc, N, M, C, accumulate);
    else
        CAPE_LAUNCH(reduce_cond_kernel, dim3(N * cgroups), dim3(256), 0, (hipStream_t)stream, gv, scale, dcond, ldc, N, M, C, accumulate);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

extern "C" int64_t cape_rowscale_reduce_workspace_bytes(int32_t N, int32_t Mo, int32_t F, int32_t R) {
    if (N < 1 || Mo < 1 || F < 1 || R < 1 || R > RSR_MAXR) return CAPE_EINVAL;
    const long long chunks = (Mo + RSR_RB - 1) / RSR_RB;
    return (int64_t)N * chunks * R * F * (int64_t)sizeof(float);
}

extern "C" int cape_rowscale_reduce(const float *dz, int64_t dz_sample_stride, int32_t lddz, const float *rowscale, int32_t R,
                                    int32_t N, int32_t Mo, int32_t F, float *out, void *workspace, int64_t workspace_bytes,
                                    void *stream) {
    if (!dz || !rowscale || !out || !workspace || N < 1 || Mo < 1 || F < 1 || R < 1 || R > RSR_MAXR || lddz < F) return CAPE_EINVAL;
    if (workspace_bytes < cape_rowscale_reduce_workspace_bytes(N, Mo, F, R)) return CAPE_EWORKSPACE;
    const int chunks = (Mo + RSR_RB - 1) / RSR_RB;
    CView zv{dz, dz_sample_stride, lddz};
    hipStream_t st = (hipStream_t)stream;
    CAPE_LAUNCH(rowscale_partial_kernel, dim3(N * chunks), dim3(256), 0, st, zv, rowscale, R, N, Mo, F, (float *)workspace, chunks);
    CAPE_LAUNCH_CHECK();
    const int RF = R * F;
    CAPE_LAUNCH(rowscale_final_kernel, dim3(N * ((RF + 63) / 64)), dim3(256), 0, st, (const float *)workspace, chunks, RF, N, out);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

extern "C" int64_t cape_bwd_prep_workspace_bytes(int32_t N, int32_t Mo, int32_t F, int32_t R) {
    if (N < 1 || Mo < 1 || F < 1 || R < 0 || R > RSR_MAXR) return CAPE_EINVAL;
    const int RB = bp_rows(N, Mo);
    const long long chunks = (Mo + RB - 1) / RB;
    return (int64_t)N * chunks * (R + 2) * F * (int64_t)sizeof(float);
}

namespace {
// The dispatch of cape_bwd_prep, decided on the host from the views alone (cape_bwd_prep_plan returns it as it stands).
struct BpPlan {
    int family, depth, RB, chunks, passes, bound;
};
template <typename T>
BpPlan bp_plan(const T *g, int64_t g_sample_stride, int32_t ldg, const T *y, int64_t y_sample_stride, int32_t ldy, int32_t act,
               const uint32_t *mask, const T *dz, int64_t dz_sample_stride, int32_t lddz, int32_t N, int32_t Mo, int32_t F, bool want_rm) {
    constexpr int es = (int)sizeof(T);
    BpPlan P;
    P.RB = bp_rows(N, Mo);
    P.chunks = (Mo + P.RB - 1) / P.RB;
    const bool vec = aligned4(g, g_sample_stride, ldg, F, es) && aligned4(dz, dz_sample_stride, lddz, F, es) &&
                     (mask || act == CAPE_ACT_NONE || aligned4(y, y_sample_stride, ldy, F, es)) &&
                     (F >= 256 ? (F % 256) == 0 : (256 % (F / 4)) == 0) && ((F & 31) == 0 || !mask);
    // 8 channels per thread where the rows allow it (column passes of 512 channels; F / 8 column groups must divide 256)
    const bool wide = vec && spmm_wide() && aligned8(g, g_sample_stride, ldg, F, es) && aligned8(dz, dz_sample_stride, lddz, F, es) &&
                      (mask || act == CAPE_ACT_NONE || aligned8(y, y_sample_stride, ldy, F, es)) &&
                      F >= 256 && (F >= 512 ? (F % 512) == 0 : (256 % (F / 8)) == 0);
    // measured (tools/bench_sparse.py, profiles/r02_ubench_sparse_bwd_prep.txt): two rows ahead is the best depth for the 4-wide
    // kernel; the 8-wide one pays only from 256 channels (fewer row lanes per column group below that), fp32 without
    // read-ahead (167 registers at depth 4, 129 at 2)
    const int ur = (wide && es == 4) ? 1 : CAPE_BP_UNROLL_DEFAULT;
    P.family = wide ? CAPE_BP_VEC8 : vec ? CAPE_BP_VEC4 : F <= 4 ? CAPE_BP_NARROW : CAPE_BP_GENERIC;
    P.depth = vec ? (ur >= 4 ? 4 : ur >= 2 ? 2 : 1) : 0;
    const int fb = wide ? 512 : vec ? 256 : P.family == CAPE_BP_NARROW ? 4 : 64;
    P.passes = (F + fb - 1) / fb;
    // bwd_prep_vec_kernel keeps one bound entry per column pass and a row has four: wider rows, and the scalar forms (which
    // do not own whole rows per lane group), take the standalone pass
    P.bound = !want_rm ? CAPE_BP_BOUND_NONE : (vec && P.passes <= 4) ? CAPE_BP_BOUND_KERNEL : CAPE_BP_BOUND_STANDALONE;
    return P;
}

template <typename T>
int bwd_prep_plan_impl(const T *g, int64_t g_sample_stride, int32_t ldg, const T *y, int64_t y_sample_stride, int32_t ldy,
                       int32_t act, const uint32_t *mask, const T *dz, int64_t dz_sample_stride, int32_t lddz, int32_t N, int32_t Mo,
                       int32_t F, int32_t want_rowmax, int32_t plan[6]) {
    if (!plan || (want_rowmax && sizeof(T) != 4)) return CAPE_EINVAL;
    if (!g || !dz || N < 1 || Mo < 1 || F < 1 || ldg < F || lddz < F) return CAPE_EINVAL;
    if (act < CAPE_ACT_NONE || act > CAPE_ACT_TANH) return CAPE_EINVAL;
    if (!mask && act != CAPE_ACT_NONE && (!y || ldy < F)) return CAPE_EINVAL;
    const BpPlan P = bp_plan<T>(g, g_sample_stride, ldg, y, y_sample_stride, ldy, act, mask, dz, dz_sample_stride, lddz, N, Mo, F,
                                want_rowmax != 0);
    plan[0] = P.family; plan[1] = P.depth; plan[2] = P.RB; plan[3] = P.chunks; plan[4] = P.passes; plan[5] = P.bound;
    return CAPE_OK;
}

template <typename T>
int bwd_prep_impl(const T *g, int64_t g_sample_stride, int32_t ldg, const T *y, int64_t y_sample_stride,
                  int32_t ldy, int32_t act, const uint32_t *mask, T *dz, int64_t dz_sample_stride, int32_t lddz,
                  float *dbias, const float *rowscale, int32_t R, float *dcoef, int32_t rg, float *dcoef_g,
                  int64_t dcoef_sample_stride, int32_t finalize, int32_t N, int32_t Mo, int32_t F, void *workspace,
                  int64_t workspace_bytes, float *rowmax_out, void *stream) {
    constexpr int es = (int)sizeof(T);
    if (rowmax_out && es != 4) return CAPE_EINVAL;
    if (!g || !dz || !workspace || N < 1 || Mo < 1 || F < 1 || ldg < F || lddz < F || R < 0 || R > RSR_MAXR) return CAPE_EINVAL;
    if (act < CAPE_ACT_NONE || act > CAPE_ACT_TANH) return CAPE_EINVAL;
    if (!mask && act != CAPE_ACT_NONE && (!y || ldy < F)) return CAPE_EINVAL;
    if ((R > 0 || dcoef_g) && !rowscale) return CAPE_EINVAL;
    if (R > 0 && !dcoef) return CAPE_EINVAL;
    if (workspace_bytes < cape_bwd_prep_workspace_bytes(N, Mo, F, R)) return CAPE_EWORKSPACE;
    const BpPlan P = bp_plan<T>(g, g_sample_stride, ldg, y, y_sample_stride, ldy, act, mask, dz, dz_sample_stride, lddz, N, Mo, F,
                                rowmax_out != nullptr);
    const int RB = P.RB, chunks = P.chunks;
    const bool vec = P.family >= CAPE_BP_VEC4, wide = P.family == CAPE_BP_VEC8;
    const int bp_ur = P.depth;
    CViewT<T> gv{g, g_sample_stride, ldg}, yv{y, y_sample_stride, ldy};
    ViewT<T> zv{dz, dz_sample_stride, lddz};
    hipStream_t st = (hipStream_t)stream;
    float *rm_kernel = P.bound == CAPE_BP_BOUND_KERNEL ? rowmax_out : nullptr;
    if (P.bound == CAPE_BP_BOUND_STANDALONE) {
        // the rows of g as they are on entry (dz may alias g): before the pass below
        const int rc = rm_standalone(g, g_sample_stride, ldg, N, Mo, F, rowmax_out, stream);
        if (rc) return rc;
    }
#define CAPE_BP_LAUNCH(VW_, UR_)                                                                                                    \
    CAPE_LAUNCH((bwd_prep_vec_kernel<T, VW_, UR_>), dim3(N * chunks), dim3(256), 0, st, gv, yv, act, mask, zv, rowscale, R, rg,     \
                dbias ? 1 : 0, dcoef_g ? 1 : 0, N, Mo, F, (float *)workspace, chunks, RB, rm_kernel)
    if (vec && wide) {
        if (bp_ur >= 4) CAPE_BP_LAUNCH(8, 4);
        else if (bp_ur >= 2) CAPE_BP_LAUNCH(8, 2);
        else CAPE_BP_LAUNCH(8, 1);
    } else if (vec) {
        if (bp_ur >= 4) CAPE_BP_LAUNCH(4, 4);
        else if (bp_ur >= 2) CAPE_BP_LAUNCH(4, 2);
        else CAPE_BP_LAUNCH(4, 1);
    }
#undef CAPE_BP_LAUNCH
    else if (F <= 4)
        CAPE_LAUNCH((bwd_prep_narrow_kernel<T>), dim3(N * chunks), dim3(256), 0, st, gv, yv, act, mask, zv, rowscale, R, rg, dbias ? 1 : 0,
                    dcoef_g ? 1 : 0, N, Mo, F, (float *)workspace, chunks, RB);
    else
        CAPE_LAUNCH((bwd_prep_kernel<T>), dim3(N * chunks), dim3(256), 0, st, gv, yv, act, mask, zv, rowscale, R, rg, dbias ? 1 : 0,
                    dcoef_g ? 1 : 0, N, Mo, F, (float *)workspace, chunks, RB);
    CAPE_LAUNCH_CHECK();
    if (finalize && (dbias || R > 0 || dcoef_g)) {
        const int fblocks = (F + 15) / 16;
        const int nblk = fblocks * (1 + N * (R + 1));
        CAPE_LAUNCH(bwd_prep_final_kernel, dim3(nblk), dim3(256), 0, st, (const float *)workspace, chunks, N, F, R, dbias, dcoef, dcoef_g,
                    dcoef_sample_stride ? (long long)dcoef_sample_stride : (long long)R * F,
                    dcoef_sample_stride ? (long long)dcoef_sample_stride : (long long)F);
        CAPE_LAUNCH_CHECK();
    }
    return CAPE_OK;
}
}  // namespace

extern "C" int cape_bwd_prep(const float *g, int64_t g_sample_stride, int32_t ldg, const float *y, int64_t y_sample_stride,
                             int32_t ldy, int32_t act, const uint32_t *mask, float *dz, int64_t dz_sample_stride, int32_t lddz,
                             float *dbias, const float *rowscale, int32_t R, float *dcoef, int32_t rg, float *dcoef_g,
                             int64_t dcoef_sample_stride, int32_t finalize, int32_t N, int32_t Mo, int32_t F, void *workspace,
                             int64_t workspace_bytes, float *rowmax_out, void *stream) {
    return bwd_prep_impl<float>(g, g_sample_stride, ldg, y, y_sample_stride, ldy, act, mask, dz, dz_sample_stride, lddz, dbias,
                                rowscale, R, dcoef, rg, dcoef_g, dcoef_sample_stride, finalize, N, Mo, F, workspace, workspace_bytes,
                                rowmax_out, stream);
}

extern "C" int cape_bwd_prep_bf16(const void *g, int64_t g_sample_stride, int32_t ldg, const void *y, int64_t y_sample_stride,
                                  int32_t ldy, int32_t act, const uint32_t *mask, void *dz, int64_t dz_sample_stride, int32_t lddz,
                                  float *dbias, const float *rowscale, int32_t R, float *dcoef, int32_t rg, float *dcoef_g,
                                  int64_t dcoef_sample_stride, int32_t finalize, int32_t N, int32_t Mo, int32_t F, void *workspace,
                                  int64_t workspace_bytes, float *rowmax_out, void *stream) {
    return bwd_prep_impl<cape_bf16>((const cape_bf16 *)g, g_sample_stride, ldg, (const cape_bf16 *)y, y_sample_stride, ldy, act, mask,
                                    (cape_bf16 *)dz, dz_sample_stride, lddz, dbias, rowscale, R, dcoef, rg, dcoef_g,
                                    dcoef_sample_stride, finalize, N, Mo, F, workspace, workspace_bytes, rowmax_out, stream);
}

extern "C" int cape_bwd_prep_plan(const float *g, int64_t g_sample_stride, int32_t ldg, const float *y, int64_t y_sample_stride,
                                  int32_t ldy, int32_t act, const uint32_t *mask, const float *dz, int64_t dz_sample_stride,
                                  int32_t lddz, int32_t N, int32_t Mo, int32_t F, int32_t want_rowmax, int32_t plan[6]) {
    return bwd_prep_plan_impl<float>(g, g_sample_stride, ldg, y, y_sample_stride, ldy, act, mask, dz, dz_sample_stride, lddz, N, Mo, F,
                                     want_rowmax, plan);
}

extern "C" int cape_bwd_prep_plan_bf16(const void *g, int64_t g_sample_stride, int32_t ldg, const void *y, int64_t y_sample_stride,
                                       int32_t ldy, int32_t act, const uint32_t *mask, const void *dz, int64_t dz_sample_stride,
                                       int32_t lddz, int32_t N, int32_t Mo, int32_t F, int32_t want_rowmax, int32_t plan[6]) {
    return bwd_prep_plan_impl<cape_bf16>((const cape_bf16 *)g, g_sample_stride, ldg, (const cape_bf16 *)y, y_sample_stride, ldy, act, mask,
                                         (const cape_bf16 *)dz, dz_sample_stride, lddz, N, Mo, F, want_rowmax, plan);
}

extern "C" int cape_bwd_prep_finalize(const cape_bwd_prep_item_t *items, int32_t nitems, void *stream) {
    if (!items || nitems < 1 || nitems > CAPE_MAX_BWD_PREP_ITEMS) return CAPE_EINVAL;
    BpFinalBatch B;
    B.n = nitems;
    int off = 0;
    for (int i = 0; i < nitems; ++i) {
        const cape_bwd_prep_item_t &t = items[i];
        if (!t.workspace || t.N < 1 || t.Mo < 1 || t.F < 1 || t.R < 0 || t.R > RSR_MAXR || (t.R > 0 && !t.dcoef)) return CAPE_EINVAL;
        const int RB = bp_rows(t.N, t.Mo);
        B.it[i].part = (const float *)t.workspace;
        B.it[i].chunks = t.chunks > 0 ? t.chunks : (t.Mo + RB - 1) / RB;
        B.it[i].N = t.N; B.it[i].F = t.F; B.it[i].R = t.R;
        B.it[i].dbias = t.dbias; B.it[i].dcoef = t.dcoef; B.it[i].dcoef_g = t.dcoef_g;
        B.it[i].cs = t.dcoef_sample_stride ? (long long)t.dcoef_sample_stride : (long long)t.R * t.F;
        B.it[i].cgs = t.dcoef_sample_stride ? (long long)t.dcoef_sample_stride : (long long)t.F;
        B.blk_off[i] = off;
        off += ((t.F + 15) / 16) * (1 + t.N * (t.R + 1));
    }
    B.blk_off[nitems] = off;
    CAPE_LAUNCH(bwd_prep_final_batch_kernel, dim3(off), dim3(256), 0, (hipStream_t)stream, B);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}
