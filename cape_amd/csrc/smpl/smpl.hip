// SMPL posing of generated clothed bodies (include/cape_hip.h, "SMPL posing"): the de-normalise / mask / add step of the
// reference's demos.py and the SMPL forward pass that demos.py runs through smplx, one mesh per call, on the CPU.
//
//   cape_smpl_dress   T = minimal + mask * (d * std + mean)                                demos.py:155-161, 207-213
//   cape_smpl_joints  joint regression, Rodrigues, pose feature, kinematic chain          demos.py:267-283, 312-326
//   cape_smpl_skin    shape + pose blend shapes and linear blend skinning                 (smplx SMPL forward, demos.py:22)
//
// Kept out of cape_amd/csrc/ itself: the benchmarked training step does not launch these kernels, and the committed PMC
// evidence is keyed by a hash of the sources in that directory alone (bench._csrc_fingerprint).
#include "smpl_shared.h"

// ---------------------------------------------------------------------------------------------------------------------
// dress: one thread per scalar of a sample's [V, 3] block
__global__ void __launch_bounds__(256) smpl_dress_kernel(const float *__restrict__ d, int64_t d_ss, const float *__restrict__ mean,
                                                         const float *__restrict__ std_, const float *__restrict__ mask,
                                                         const float *__restrict__ minimal, float *__restrict__ T, int64_t T_ss,
                                                         int32_t V3) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V3) return;
    const int64_t n = blockIdx.y;
    const float x = d[n * d_ss + i] * std_[i] + mean[i];
    T[n * T_ss + i] = minimal[i] + mask[i / 3] * x;
}

// ---------------------------------------------------------------------------------------------------------------------
// joints + chain: one workgroup of 256 threads per sample
__global__ void __launch_bounds__(256) smpl_joints_kernel(const float *__restrict__ T, int64_t T_ss, const int32_t *__restrict__ rp,
                                                          const int32_t *__restrict__ ci, const float *__restrict__ cv,
                                                          const float *__restrict__ pose, const float *__restrict__ betas, int32_t B,
                                                          const float *__restrict__ jsd, const float *__restrict__ transl,
                                                          SmplTree tree, float *__restrict__ coef, float *__restrict__ G,
                                                          float *__restrict__ joints) {
    __shared__ float sJ[SMPL_MAX_J][3];
    __shared__ float sR[SMPL_MAX_J][9];
    __shared__ float sA[SMPL_MAX_J][12];        // [rot 3x3 row-major | t]
    const int32_t J = tree.J, n = blockIdx.x, tid = threadIdx.x;
    const float *bn = betas + (int64_t)n * B;
    smpl_chain(T + n * T_ss, rp, ci, cv, pose + (int64_t)n * 3 * J, bn, B, jsd, tree, sJ, sR, sA);
    const int32_t K = B + 9 * (J - 1);
    float *cn = coef + (int64_t)n * K;
    for (int32_t b = tid; b < B; b += 256) cn[b] = bn[b];
    if (tid > 0 && tid < J) {      // pose feature R_j - I, [(j-1)*9 + 3r + c]
#pragma unroll
        for (int32_t q = 0; q < 9; ++q) cn[B + (tid - 1) * 9 + q] = sR[tid][q] - ((q % 4 == 0) ? 1.f : 0.f);
    }
    // G_j = [A.rot | A.t - A.rot J_j], posed joints A.t + transl
    if (tid < J) {
        float *g = G + ((int64_t)n * J + tid) * 12;
#pragma unroll
        for (int32_t r = 0; r < 3; ++r) {
            const float a0 = sA[tid][4 * r], a1 = sA[tid][4 * r + 1], a2 = sA[tid][4 * r + 2], t = sA[tid][4 * r + 3];
            g[4 * r] = a0; g[4 * r + 1] = a1; g[4 * r + 2] = a2;
            g[4 * r + 3] = t - (a0 * sJ[tid][0] + a1 * sJ[tid][1] + a2 * sJ[tid][2]);
            if (joints) joints[((int64_t)n * J + tid) * 3 + r] = t + (transl ? transl[3 * n + r] : 0.f);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// skin: one thread per vertex, `tile` samples per workgroup of 64 or 256 threads; coef [K][tile] and G [tile][J][12] in LDS
__global__ void __launch_bounds__(256) smpl_skin_kernel(const float *__restrict__ T, int64_t T_ss, const float *__restrict__ basis,
                                                        int32_t K, const float *__restrict__ coef, const float *__restrict__ G,
                                                        const int32_t *__restrict__ ell_j, const float *__restrict__ ell_w,
                                                        int32_t W, const float *__restrict__ transl, int32_t J, int32_t V,
                                                        int32_t N, int32_t tile, float *__restrict__ out, int64_t out_ss) {
    extern __shared__ float lds[];
    float *sC = lds;                              // [K][tile]: one k of every sample of the tile is one broadcast read
    float *sG = lds + ((K * tile + 3) & ~3);      // [tile][J][12], 16-byte aligned
    const int32_t n0 = blockIdx.y * tile, ns = min(tile, N - n0);
    const int32_t nt = blockDim.x;
    for (int32_t i = threadIdx.x; i < K * ns; i += nt) {
        const int32_t s = i / K, k = i - s * K;
        sC[k * tile + s] = coef[(int64_t)(n0 + s) * K + k];
    }
    for (int32_t i = threadIdx.x; i < 12 * J * ns; i += nt) sG[i] = G[(int64_t)n0 * 12 * J + i];
    __syncthreads();
    const int32_t v = blockIdx.x * nt + threadIdx.x;
    if (v >= V) return;

    float acc[SMPL_TILE][3];
#pragma unroll
    for (int32_t s = 0; s < SMPL_TILE; ++s) acc[s][0] = acc[s][1] = acc[s][2] = 0.f;
    // the blend basis [K][3][V] streamed once for the whole tile
#pragma unroll 2
    for (int32_t k = 0; k < K; ++k) {
        const float bx = basis[(3 * k) * V + v], by = basis[(3 * k + 1) * V + v], bz = basis[(3 * k + 2) * V + v];
        const float *c = sC + k * tile;
#pragma unroll
        for (int32_t s = 0; s < SMPL_TILE; ++s) {
            if (s < ns) {
                const float w = c[s];
                acc[s][0] += w * bx; acc[s][1] += w * by; acc[s][2] += w * bz;
            }
        }
    }
#pragma unroll
    for (int32_t s = 0; s < SMPL_TILE; ++s) {
        if (s >= ns) continue;              // ns is uniform: a scalar branch; `break` would defeat the unroll
        const int64_t n = n0 + s;
        const float *t = T + n * T_ss + 3 * v;
        const float px = t[0] + acc[s][0], py = t[1] + acc[s][1], pz = t[2] + acc[s][2];
        // M = sum_w weight * G[joint]: the skinning weights' nonzeros in increasing joint order
        float M[12];
#pragma unroll
        for (int32_t q = 0; q < 12; ++q) M[q] = 0.f;
        for (int32_t w = 0; w < W; ++w) {
            const float a = ell_w[w * V + v];
            const float4 *g = reinterpret_cast<const float4 *>(sG + (s * J + ell_j[w * V + v]) * 12);
            const float4 g0 = g[0], g1 = g[1], g2 = g[2];
            M[0] += a * g0.x; M[1] += a * g0.y; M[2] += a * g0.z;  M[3] += a * g0.w;
            M[4] += a * g1.x; M[5] += a * g1.y; M[6] += a * g1.z;  M[7] += a * g1.w;
            M[8] += a * g2.x; M[9] += a * g2.y; M[10] += a * g2.z; M[11] += a * g2.w;
        }
        float *o = out + n * out_ss + 3 * v;
#pragma unroll
        for (int32_t r = 0; r < 3; ++r)
            o[r] = M[4 * r] * px + M[4 * r + 1] * py + M[4 * r + 2] * pz + M[4 * r + 3] + (transl ? transl[3 * n + r] : 0.f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
extern "C" int cape_smpl_dress(const float *disp, int64_t disp_sample_stride, const float *mean, const float *std_,
                               const float *mask, const float *minimal, float *T, int64_t T_sample_stride, int32_t N,
                               int32_t V, void *stream) {
    if (!disp || !mean || !std_ || !mask || !minimal || !T) return CAPE_EINVAL;
    if (N < 1 || N > 65535 || V < 1 || V > (1 << 29)) return CAPE_EINVAL;
    if (disp_sample_stride < 3LL * V || T_sample_stride < 3LL * V) return CAPE_EINVAL;
    dim3 grid((3 * V + 255) / 256, N);
    smpl_dress_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(disp, disp_sample_stride, mean, std_, mask, minimal, T,
                                                              T_sample_stride, 3 * V);
    return launch_status();
}

extern "C" int cape_smpl_joints(const float *T, int64_t T_sample_stride, const int32_t *jreg_rowptr,
                                const int32_t *jreg_colidx, const float *jreg_vals, const float *pose, const float *betas,
                                int32_t B, const float *jshapedirs, const float *transl, const int32_t *parents, int32_t J,
                                int32_t V, int32_t N, float *coef, float *G, float *joints, void *stream) {
    SmplTree tree;
    const int rc = smpl_tree(parents, J, &tree);
    if (rc) return rc;
    if (!T || !jreg_rowptr || !jreg_colidx || !jreg_vals || !pose || !coef || !G) return CAPE_EINVAL;
    if (B < 0 || (B > 0 && (!betas || !jshapedirs))) return CAPE_EINVAL;
    if (N < 1 || V < 1 || V > (1 << 29) || T_sample_stride < 0 || (T_sample_stride > 0 && T_sample_stride < 3LL * V))
        return CAPE_EINVAL;
    smpl_joints_kernel<<<N, 256, 0, (hipStream_t)stream>>>(T, T_sample_stride, jreg_rowptr, jreg_colidx, jreg_vals, pose, betas,
                                                           B, jshapedirs, transl, tree, coef, G, joints);
    return launch_status();
}

extern "C" int cape_smpl_skin_tile(int32_t K, int32_t J) {
    if (K < 0 || J < 1 || J > SMPL_MAX_J) return CAPE_EINVAL;
    const int64_t per_sample = 4LL * K + 48LL * J;
    const int64_t t = (SMPL_SKIN_LDS - 16) / per_sample;           // 16: the alignment pad in front of the G block
    return t < 1 ? CAPE_EINVAL : (int)(t < SMPL_TILE ? t : SMPL_TILE);
}

extern "C" int cape_smpl_skin(const float *T, int64_t T_sample_stride, const float *basis, int32_t K, const float *coef,
                              const float *G, const int32_t *ell_joint, const float *ell_weight, int32_t ell_width,
                              const float *transl, int32_t J, int32_t V, int32_t N, float *out, int64_t out_sample_stride,
                              void *stream) {
    const int tile = cape_smpl_skin_tile(K, J);
    if (tile < 0) return tile;
    if (!T || (K > 0 && (!basis || !coef)) || !G || !ell_joint || !ell_weight || !out) return CAPE_EINVAL;
    if (N < 1 || V < 1 || ell_width < 1 || ell_width > J) return CAPE_EINVAL;
    if (3LL * K * V >= (1LL << 31) || (int64_t)ell_width * V >= (1LL << 31)) return CAPE_EINVAL;   // 32-bit element index
    if (T_sample_stride < 0 || (T_sample_stride > 0 && T_sample_stride < 3LL * V) || out_sample_stride < 3LL * V)
        return CAPE_EINVAL;
    const int32_t tiles = (N + tile - 1) / tile;
    if (tiles > 65535) return CAPE_EINVAL;
    // 256-thread workgroups once they fill the chip; below that one wave each, four times as many workgroups to stream with
    const int32_t threads = (int64_t)tiles * ((V + 255) / 256) >= 256 ? 256 : 64;
    dim3 grid((V + threads - 1) / threads, tiles);
    const size_t lds = 4 * (size_t)(((K * tile + 3) & ~3) + 12 * J * tile);
    smpl_skin_kernel<<<grid, threads, lds, (hipStream_t)stream>>>(T, T_sample_stride, basis, K, coef, G, ell_joint, ell_weight,
                                                              ell_width, transl, J, V, N, tile, out, out_sample_stride);
    return launch_status();
}
