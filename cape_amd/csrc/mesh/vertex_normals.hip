// Per-vertex normals of a batch of triangle meshes and their gradient: the reference's estimate_vertex_normals
// (lib/losses.py:54-80, its restatement of psbody.mesh's routine on lib/utils.py:119-135 TriNormals / NormalizedNx3), which
// nothing in the reference calls.  For vertices x [V, 3] and faces (i0, i1, i2):
//   m_f = (x[i1] - x[i0]) x (x[i2] - x[i0]);  u_f = m_f / sqrt(m_f.m_f + [m_f.m_f == 0])      (a degenerate face: 0)
//   s_v = sum of u_f over the faces that use v   (UNIFORM weights, not area weights: summing m_f instead would be that variant)
//   n_v = s_v / sqrt(s_v.s_v + [s_v.s_v == 0])   (no faces, or unit normals that cancel: 0)
// Gradient with both masks constant (what autograd gives for the expression as written), gbar = dL/dn:
//   h_v = (gbar_v - n_v (n_v.gbar_v)) / |s_v|';  G_f = h_i0 + h_i1 + h_i2;  gamma_f = (G_f - u_f (u_f.G_f)) / |m_f|'
//   dL/dx[corner k of f] += gamma_f x (x[k+2] - x[k+1])      (corners cyclic: the edge opposite the corner; ' = the guarded root)
// One work item per (sample, vertex) walks the vertex's incident (face, corner) list (graph.vertex_face_table) in list order and
// recomputes each face's unit normal from its three corners: no face-normal array in memory, no atomics, fixed-order sums.
// The arithmetic between the fp32 loads and the fp32 stores is fp64 (half the fp32 vector peak on this part, and the kernels
// wait on their gathers): s_v is a sum of unit vectors that partly cancel, and the error of fp32 face normals is amplified by
// 1 / |s_v| in n and by 1 / (|s_v| |m_f|) in the gradient.
#include "../common.h"

namespace {

constexpr int LB = 256;
constexpr int MAXB = 1024;

struct d3 {
    double x, y, z;
};

__device__ __forceinline__ d3 load3(const float *p) { return {(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ d3 sub(d3 a, d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ d3 add(d3 a, d3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ double dot(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ d3 cross(d3 a, d3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ d3 scale(d3 a, double k) { return {a.x * k, a.y * k, a.z * k}; }

// a / sqrt(a.a + [a.a == 0]) in place; returns 1 / that root
__device__ __forceinline__ double normalize(d3 &a) {
    const double ss = dot(a, a);
    const double inv = 1.0 / sqrt(ss + (ss == 0.0 ? 1.0 : 0.0));
    a = scale(a, inv);
    return inv;
}

// the unit normal of face f of the sample whose rows start at xs; inv_m = 1 / |m_f|'; p[k] = corner k
__device__ __forceinline__ d3 face_unit(const float *xs, int ldx, const int *faces, int f, d3 (&p)[3], double &inv_m) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = load3(xs + (long long)faces[3 * f + k] * ldx);
    d3 m = cross(sub(p[1], p[0]), sub(p[2], p[0]));
    inv_m = normalize(m);
    return m;
}

// s_v, summed in list order
__device__ __forceinline__ d3 vertex_sum(const float *xs, int ldx, const int *faces, const int *vidx, int t0, int t1) {
    d3 s = {0.0, 0.0, 0.0};
    for (int t = t0; t < t1; ++t) {
        d3 p[3];
        double inv_m;
        s = add(s, face_unit(xs, ldx, faces, vidx[t] / 3, p, inv_m));
    }
    return s;
}

// forward: n [N, V, ldn];  with gbar: h [N, V, 3] instead (the backward's first launch)
template <bool H>
__global__ __launch_bounds__(LB) void vertex_normal_kernel(const float *x, int ldx, const float *gbar, int ldg, const int *faces,
                                                           const int *vptr, const int *vidx, int N, int V, float *out, int ldo) {
    const long long total = (long long)N * V;
    for (long long i = (long long)blockIdx.x * LB + threadIdx.x; i < total; i += (long long)gridDim.x * LB) {
        const int v = (int)(i % V);
        const long long n = i / V;
        d3 s = vertex_sum(x + n * V * ldx, ldx, faces, vidx, vptr[v], vptr[v + 1]);
        const double inv_s = normalize(s);                     // s is n_v from here on
        if constexpr (H) {
            const d3 g = load3(gbar + i * ldg);
            s = scale(sub(g, scale(s, dot(s, g))), inv_s);
        }
        float *o = out + i * ldo;
        o[0] = (float)s.x;
        o[1] = (float)s.y;
        o[2] = (float)s.z;
    }
}

// the backward's second launch: per (n, v), over its incident corners in list order, gamma_f x (the opposite edge)
__global__ __launch_bounds__(LB) void vertex_normal_grad_kernel(const float *x, int ldx, const float *h, const int *faces,
                                                                const int *vptr, const int *vidx, int N, int V, float *dx, int ldd) {
    const long long total = (long long)N * V;
    for (long long i = (long long)blockIdx.x * LB + threadIdx.x; i < total; i += (long long)gridDim.x * LB) {
        const int v = (int)(i % V);
        const long long n = i / V;
        const float *xs = x + n * V * ldx, *hs = h + n * V * 3;
        d3 acc = {0.0, 0.0, 0.0};
        for (int t = vptr[v]; t < vptr[v + 1]; ++t) {
            const int code = vidx[t];
            const int f = code / 3, k = code - 3 * f;
            d3 p[3];
            double inv_m;
            const d3 u = face_unit(xs, ldx, faces, f, p, inv_m);
            const d3 G = add(add(load3(hs + (long long)faces[3 * f] * 3), load3(hs + (long long)faces[3 * f + 1] * 3)),
                             load3(hs + (long long)faces[3 * f + 2] * 3));
            const d3 gamma = scale(sub(G, scale(u, dot(u, G))), inv_m);
            // x[k+2] - x[k+1] without indexing p at run time
            const d3 e = k == 0 ? sub(p[2], p[1]) : (k == 1 ? sub(p[0], p[2]) : sub(p[1], p[0]));
            acc = add(acc, cross(gamma, e));
        }
        float *o = dx + i * ldd;
        o[0] = (float)acc.x;
        o[1] = (float)acc.y;
        o[2] = (float)acc.z;
    }
}

// work-item and table indices are int32: N V and 3 F stay below 2^31
inline bool sizes_ok(int64_t N, int64_t V, int64_t F) {
    return N >= 1 && V >= 1 && F >= 1 && N * V < ((int64_t)1 << 31) && 3 * F < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int64_t cape_vertex_normals_workspace_bytes(int32_t N, int32_t V) {
    if (!sizes_ok(N, V, 1)) return CAPE_EINVAL;
    return (int64_t)N * V * 3 * (int64_t)sizeof(float);
}

extern "C" int cape_vertex_normals_fwd(const float *x, int32_t ldx, const int32_t *faces, const int32_t *vert_face_ptr,
                                       const int32_t *vert_face_idx, int32_t N, int32_t V, int32_t F, float *normals, int32_t ldn,
                                       void *stream) {
    if (!x || !faces || !vert_face_ptr || !vert_face_idx || !normals) return CAPE_EINVAL;
    if (!sizes_ok(N, V, F) || ldx < 3 || ldn < 3) return CAPE_EINVAL;
    CAPE_LAUNCH(vertex_normal_kernel<false>, dim3(cape_grid_blocks((long long)N * V, LB, MAXB)), dim3(LB), 0, (hipStream_t)stream, x,
                ldx, (const float *)nullptr, 0, faces, vert_face_ptr, vert_face_idx, N, V, normals, ldn);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}

extern "C" int cape_vertex_normals_bwd(const float *x, int32_t ldx, const float *gnormals, int32_t ldg, const int32_t *faces,
                                       const int32_t *vert_face_ptr, const int32_t *vert_face_idx, int32_t N, int32_t V, int32_t F,
                                       float *dx, int32_t ldd, void *workspace, int64_t workspace_bytes, void *stream) {
    if (!x || !gnormals || !faces || !vert_face_ptr || !vert_face_idx || !dx || !workspace) return CAPE_EINVAL;
    if (!sizes_ok(N, V, F) || ldx < 3 || ldg < 3 || ldd < 3) return CAPE_EINVAL;
    if (workspace_bytes < cape_vertex_normals_workspace_bytes(N, V)) return CAPE_EINVAL;
    float *h = (float *)workspace;
    hipStream_t st = (hipStream_t)stream;
    const int nb = cape_grid_blocks((long long)N * V, LB, MAXB);
    CAPE_LAUNCH(vertex_normal_kernel<true>, dim3(nb), dim3(LB), 0, st, x, ldx, gnormals, ldg, faces, vert_face_ptr, vert_face_idx, N,
                V, h, 3);
    CAPE_LAUNCH_CHECK();
    CAPE_LAUNCH(vertex_normal_grad_kernel, dim3(nb), dim3(LB), 0, st, x, ldx, (const float *)h, faces, vert_face_ptr, vert_face_idx,
                N, V, dx, ldd);
    CAPE_LAUNCH_CHECK();
    return CAPE_OK;
}
