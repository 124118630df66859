// Per-vertex weighted reconstruction loss + SMPL edge loss and their gradients w.r.t. the prediction: the reference's
// loss_mask option (lib/models.py:47-52, 357-369), the mask handed to tf.losses.*(weights=...) with Reduction.MEAN:
//   recon = sum w * l(pred - gt) / sum w       (w the [V, 3] weights broadcast over the batch; the host passes 1 / sum w)
//   l = |d| (l1), 0.5 d^2 if |d| <= 0.1 else 0.1 |d| - 0.005 (huber), d^2 (l2)
//   d recon / d pred = w * l'(d) / sum w,  l'(0) = 0 for l1 (TF's sign), l'(d) = clip(d, -0.1, 0.1) for huber
// The edge loss is csrc/loss.hip's, restated with the same arithmetic and reduction order (its kernels are file-local), so
// the edge value and the edge part of the gradient equal the unmasked kernel's bits.  Fixed-order sums, no atomics.
#include <cmath>

#include "../common.h"

namespace {

constexpr int LB = 256;

__device__ __forceinline__ float block_sum256(float v, float *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// per (n, e): unit difference vector -> unit[n,e,0:3], block-partial sum of lengths (loss.hip edge_fwd_kernel)
__global__ __launch_bounds__(LB) void masked_edge_kernel(const float *pred, const float *gt, const float *ref, const int *edges,
                                                         int N, int M, int E, int ldp, float *unit, float *part) {
    __shared__ float red[4];
    const long long total = (long long)N * E;
    float s = 0.f;
    for (long long i = (long long)blockIdx.x * LB + threadIdx.x; i < total; i += (long long)gridDim.x * LB) {
        const int e = (int)(i % E);
        const long long n = i / E;
        const int a = edges[2 * e], b = edges[2 * e + 1];
        float d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float pa = pred[(n * M + a) * ldp + k] + ref[a * 3 + k];
            const float pb = pred[(n * M + b) * ldp + k] + ref[b * 3 + k];
            const float ga = gt[(n * M + a) * 3 + k] + ref[a * 3 + k];
            const float gb = gt[(n * M + b) * 3 + k] + ref[b * 3 + k];
            d[k] = (pa - pb) - (ga - gb);
        }
        const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        s += len;
        const float inv = len > 0.f ? 1.f / len : 0.f;
        if (unit) {
            unit[i * 3 + 0] = d[0] * inv;
            unit[i * 3 + 1] = d[1] * inv;
            unit[i * 3 + 2] = d[2] * inv;
        }
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// loss value l(d) and slope l'(d) of one coordinate; KIND 0 = l1, 1 = huber (delta 0.1), 2 = l2
template <int KIND>
__device__ __forceinline__ void pointwise_loss(float d, float &l, float &dl) {
    if (KIND == 0) {
        l = fabsf(d);
        dl = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    } else if (KIND == 1) {
        const float a = fabsf(d);
        l = a <= 0.1f ? 0.5f * a * a : 0.1f * a - 0.005f;
        dl = fminf(fmaxf(d, -0.1f), 0.1f);
    } else {
        l = d * d;
        dl = 2.f * d;
    }
}

// per (n, v): weighted partial sums and the combined gradient; cr = w_recon / sum w
template <int KIND>
__global__ __launch_bounds__(LB) void masked_vert_kernel(const float *pred, const float *gt, const float *wts, const float *unit,
                                                         const int *vptr, const int *vidx, int N, int M, int E, int ldp, int ldd,
                                                         float cr, float ce, float *dpred, float *part) {
    __shared__ float red[4];
    const long long total = (long long)N * M;
    float s = 0.f;
    for (long long i = (long long)blockIdx.x * LB + threadIdx.x; i < total; i += (long long)gridDim.x * LB) {
        const int v = (int)(i % M);
        const long long n = i / M;
        float g[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float d = pred[i * ldp + k] - gt[i * 3 + k];
            const float w = wts[v * 3 + k];
            float l, dl;
            pointwise_loss<KIND>(d, l, dl);
            s = fmaf(w, l, s);
            g[k] = cr * (w * dl);
        }
        if (dpred) {
            for (int t = vptr[v]; t < vptr[v + 1]; ++t) {
                const int code = vidx[t];
                const int e = code >> 1;
                const float sg = (code & 1) ? -ce : ce;
                const float *u = unit + (n * E + e) * 3;
                g[0] = fmaf(sg, u[0], g[0]);
                g[1] = fmaf(sg, u[1], g[1]);
                g[2] = fmaf(sg, u[2], g[2]);
            }
            dpred[i * ldd + 0] = g[0];
            dpred[i * ldd + 1] = g[1];
            dpred[i * ldd + 2] = g[2];
        }
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one block: both sums in a fixed order (the edge one exactly as loss.hip loss_final_kernel), the weighted total
__global__ __launch_bounds__(LB) void masked_final_kernel(const float *part_e, int ne, float inv_e, const float *part_v, int nv,
                                                          float inv_w, float *loss_out, float w_recon, float w_edge, float *total_out,
                                                          const float *term_a, float w_a, const float *term_b) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < nv; i += LB) s += part_v[i];
    s = block_sum256(s, red);
    float t = 0.f;
    for (int i = threadIdx.x; i < ne; i += LB) t += part_e[i];
    t = block_sum256(t, red);
    if (threadIdx.x == 0) {
        loss_out[0] = s * inv_w;
        loss_out[1] = t * inv_e;
        if (total_out) {
            float tot = w_recon * (s * inv_w) + w_edge * (t * inv_e);
            if (term_a) tot = fmaf(w_a, *term_a, tot);
            if (term_b) tot += *term_b;
            *total_out = tot;
        }
    }
}

inline int nblocks(long long total) {
    long long b = (total + LB - 1) / LB;
    if (b > 1024) b = 1024;
    return (int)(b < 1 ? 1 : b);
}

}  // namespace

extern "C" int64_t cape_masked_recon_edge_workspace_bytes(int32_t N, int32_t M, int32_t E) {
    if (N < 1 || M < 1 || E < 1) return CAPE_EINVAL;
    return ((int64_t)N * E * 3 + 2048) * (int64_t)sizeof(float);
}

extern "C" int cape_masked_recon_edge_loss_fwd_bwd(const float *pred, int32_t ldp, const float *gt, const float *verts_ref,
                                                   const int32_t *edges, const int32_t *vert_edge_ptr, const int32_t *vert_edge_idx,
                                                   int32_t N, int32_t M, int32_t E, const float *weights, int32_t loss_kind,
                                                   float inv_weight_sum, float w_recon, float w_edge, float *loss_out,
                                                   float *total_out, const float *term_a, float w_a, const float *term_b,
                                                   float *dpred, int32_t ldd, void *workspace, int64_t workspace_bytes, void *stream) {
    if (!pred || !gt || !verts_ref || !edges || !weights || !loss_out || !workspace || N < 1 || M < 1 || E < 1 || ldp < 3)
        return CAPE_EINVAL;
    if (loss_kind < 0 || loss_kind > 2) return CAPE_EINVAL;
    if (!(inv_weight_sum > 0.f) || !std::isfinite(inv_weight_sum)) return CAPE_EINVAL;    // sum w > 0 and finite
    if (dpred && ldd < 3) return CAPE_EINVAL;
    if (dpred && (!vert_edge_ptr || !vert_edge_idx)) return CAPE_EINVAL;
    if (workspace_bytes < cape_masked_recon_edge_workspace_bytes(N, M, E)) return CAPE_EWORKSPACE;
    float *ws = (float *)workspace;
    float *part_e = ws, *part_v = ws + 1024, *unit = ws + 2048;
    hipStream_t st = (hipStream_t)stream;
    const int ne = nblocks((long long)N * E), nv = nblocks((long long)N * M);
    CAPE_LAUNCH(masked_edge_kernel, dim3(ne), dim3(LB), 0, st, pred, gt, verts_ref, edges, N, M, E, ldp, unit, part_e);
    CAPE_LAUNCH_CHECK();
    const float cr = w_recon * inv_weight_sum;
    const float ce = w_edge / ((float)N * (float)E);
    switch (loss_kind) {
        case 0:
            CAPE_LAUNCH(masked_vert_kernel<0>, dim3(nv), dim3(LB), 0, st, pred, gt, weights, unit, vert_edge_ptr, vert_edge_idx, N, M,
                        E, ldp, ldd, cr, ce, dpred, part_v);
            break;
        case 1:
            CAPE_LAUNCH(masked_vert_kernel<1>, dim3(nv), dim3(LB), 0, st, pred, gt, weights, unit, vert_edge_ptr, vert_edge_idx, N, M,
                        E, ldp, ldd, cr, ce, dpred, part_v);
            break;
        default:
            CAPE_LAUNCH(masked_vert_kernel<2>, dim3(nv), dim3(LB), 0, st, pred, gt, weights, unit, vert_edge_ptr, vert_edge_idx, N, M,
                        E, ldp, ldd, cr, ce, dpred, part_v);
            break;
    }
    CAPE_LAUNCH_CHECK();
    CAPE_LAUNCH(masked_final_kernel, dim3(1), dim3(LB), 0, st, part_e, ne, 1.0f / ((float)N * (float)E), part_v, nv, inv_weight_sum,
                loss_out, w_recon, w_edge, total_out, term_a, w_a, term_b);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}
