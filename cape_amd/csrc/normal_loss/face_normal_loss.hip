// Face-normal loss and its gradient w.r.t. the prediction: the reference's face_normal_loss_calc (lib/losses.py:27-52, on
// lib/utils.py:119-135 TriNormals / NormalizedNx3), which its lib/models.py never wires in (the "+ 0." slot of :393-395).
//   x = pred + verts_ref, y = gt + verts_ref;  face (i0, i1, i2):  m(x) = (x[i1] - x[i0]) x (x[i2] - x[i0])
//   n(x) = m / sqrt(ss + [ss == 0]), ss = m.m  (zero guard, no epsilon);  c = n(x).n(y);  normal = mean over N*F of 1 - |c|
//   d normal / d m = -sign(c) (n(y) - c n(x)) / |m| / (N F) =: g,  sign(0) = 0
//   d / d x[corner k] = g x (x[k+2] - x[k+1])   (corners cyclic: the edge opposite the corner)
// Edge vectors are formed as (pred[j] - pred[i]) + (ref[j] - ref[i]): the same number as x[j] - x[i] without first rounding
// each sum to fp32 (the template is ~50x larger than a clothing offset).  Fixed-order sums, no atomics.
#include <cmath>

#include "../common.h"

namespace {

constexpr int LB = 256;
constexpr int MAXB = 1024;

__device__ __forceinline__ void cross3(const float *a, const float *b, float *m) {
    m[0] = a[1] * b[2] - a[2] * b[1];
    m[1] = a[2] * b[0] - a[0] * b[2];
    m[2] = a[0] * b[1] - a[1] * b[0];
}

// m / sqrt(ss + [ss == 0]) in place; returns 1 / that root
__device__ __forceinline__ float normalize3(float *m) {
    const float ss = m[0] * m[0] + m[1] * m[1] + m[2] * m[2];
    const float inv = 1.f / sqrtf(ss + (ss == 0.f ? 1.f : 0.f));
    m[0] *= inv;
    m[1] *= inv;
    m[2] *= inv;
    return inv;
}

// per (n, f): 1 - |c| into the block's partial sum; g[n, f, 0:3] (scaled by coef = w_normal / (N F)) when asked
__global__ __launch_bounds__(LB) void normal_face_kernel(const float *pred, const float *gt, const float *ref, const int *faces,
                                                         int N, int M, int F, int ldp, float coef, float *g, float *part) {
    __shared__ float red[4];
    const long long total = (long long)N * F;
    float s = 0.f;
    for (long long i = (long long)blockIdx.x * LB + threadIdx.x; i < total; i += (long long)gridDim.x * LB) {
        const int f = (int)(i % F);
        const long long n = i / F;
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        const float *p0 = pred + (n * M + i0) * ldp, *p1 = pred + (n * M + i1) * ldp, *p2 = pred + (n * M + i2) * ldp;
        const float *q0 = gt + (n * M + i0) * 3, *q1 = gt + (n * M + i1) * 3, *q2 = gt + (n * M + i2) * 3;
        float a[3], b[3], ay[3], by[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float r0 = ref[i0 * 3 + k];
            const float ra = ref[i1 * 3 + k] - r0, rb = ref[i2 * 3 + k] - r0;
            a[k] = (p1[k] - p0[k]) + ra;
            b[k] = (p2[k] - p0[k]) + rb;
            ay[k] = (q1[k] - q0[k]) + ra;
            by[k] = (q2[k] - q0[k]) + rb;
        }
        float nx[3], ny[3];
        cross3(a, b, nx);
        cross3(ay, by, ny);
        const float inv = normalize3(nx);
        normalize3(ny);
        const float c = nx[0] * ny[0] + nx[1] * ny[1] + nx[2] * ny[2];
        s += 1.f - fabsf(c);
        if (g) {
            const float sg = c > 0.f ? -coef : (c < 0.f ? coef : 0.f);      // -sign(c) coef
            const float k = sg * inv;
            g[i * 3 + 0] = k * (ny[0] - c * nx[0]);
            g[i * 3 + 1] = k * (ny[1] - c * nx[1]);
            g[i * 3 + 2] = k * (ny[2] - c * nx[2]);
        }
    }
    s = cape_block_sum256(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// per (n, v): sum over the vertex's incident (face, corner) list, in list order, of g[n, f] x (opposite edge)
__global__ __launch_bounds__(LB) void normal_vert_kernel(const float *pred, const float *ref, const int *faces, const int *vptr,
                                                         const int *vidx, const float *g, int N, int M, int F, int ldp, int ldd,
                                                         float *dpred) {
    const long long total = (long long)N * M;
    for (long long i = (long long)blockIdx.x * LB + threadIdx.x; i < total; i += (long long)gridDim.x * LB) {
        const int v = (int)(i % M);
        const long long n = i / M;
        float acc[3] = {0.f, 0.f, 0.f};
        for (int t = vptr[v]; t < vptr[v + 1]; ++t) {
            const int code = vidx[t];
            const int f = code / 3, k = code - 3 * f;
            const int j1 = faces[3 * f + (k == 2 ? 0 : k + 1)], j2 = faces[3 * f + (k == 0 ? 2 : k - 1)];
            const float *p1 = pred + (n * M + j1) * ldp, *p2 = pred + (n * M + j2) * ldp;
            float e[3], d[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) e[q] = (p2[q] - p1[q]) + (ref[j2 * 3 + q] - ref[j1 * 3 + q]);
            cross3(g + (n * F + f) * 3, e, d);
            acc[0] += d[0];
            acc[1] += d[1];
            acc[2] += d[2];
        }
        dpred[i * ldd + 0] = acc[0];
        dpred[i * ldd + 1] = acc[1];
        dpred[i * ldd + 2] = acc[2];
    }
}

// one block: the partial sums in a fixed order, the mean, the weighted total
__global__ __launch_bounds__(LB) void normal_final_kernel(const float *part, int nb, float inv_nf, float w_normal, float *loss_out,
                                                          float *total_out, const float *term_in) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < nb; i += LB) s += part[i];
    s = cape_block_sum256(s, red);
    if (threadIdx.x == 0) {
        const float normal = s * inv_nf;
        loss_out[0] = normal;
        if (total_out) *total_out = fmaf(w_normal, normal, term_in ? *term_in : 0.f);
    }
}

}  // namespace

extern "C" int64_t cape_face_normal_loss_workspace_bytes(int32_t N, int32_t M, int32_t F) {
    if (N < 1 || M < 1 || F < 1) return CAPE_EINVAL;
    return ((int64_t)N * F * 3 + MAXB) * (int64_t)sizeof(float);
}

extern "C" int cape_face_normal_loss_fwd_bwd(const float *pred, int32_t ldp, const float *gt, const float *verts_ref,
                                             const int32_t *faces, const int32_t *vert_face_ptr, const int32_t *vert_face_idx,
                                             int32_t N, int32_t M, int32_t F, float w_normal, float *loss_out, float *total_out,
                                             const float *term_in, float *dpred, int32_t ldd, void *workspace,
                                             int64_t workspace_bytes, void *stream) {
    if (!pred || !gt || !verts_ref || !faces || !loss_out || !workspace || N < 1 || M < 1 || F < 1 || ldp < 3) return CAPE_EINVAL;
    if (!std::isfinite(w_normal)) return CAPE_EINVAL;
    if (term_in && !total_out) return CAPE_EINVAL;
    if (dpred && ldd < 3) return CAPE_EINVAL;
    if (dpred && (!vert_face_ptr || !vert_face_idx)) return CAPE_EINVAL;
    if (workspace_bytes < cape_face_normal_loss_workspace_bytes(N, M, F)) return CAPE_EWORKSPACE;
    float *part = (float *)workspace, *g = part + MAXB;
    hipStream_t st = (hipStream_t)stream;
    const int nf = cape_grid_blocks((long long)N * F, LB, MAXB);
    const float inv_nf = 1.0f / ((float)N * (float)F);
    CAPE_LAUNCH(normal_face_kernel, dim3(nf), dim3(LB), 0, st, pred, gt, verts_ref, faces, N, M, F, ldp, w_normal * inv_nf,
                dpred ? g : (float *)nullptr, part);
    CAPE_LAUNCH_CHECK();
    if (dpred) {
        CAPE_LAUNCH(normal_vert_kernel, dim3(cape_grid_blocks((long long)N * M, LB, MAXB)), dim3(LB), 0, st, pred, verts_ref, faces,
                    vert_face_ptr, vert_face_idx, g, N, M, F, ldp, ldd, dpred);
        CAPE_LAUNCH_CHECK();
    }
    CAPE_LAUNCH(normal_final_kernel, dim3(1), dim3(LB), 0, st, part, nf, inv_nf, w_normal, loss_out, total_out, term_in);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}
