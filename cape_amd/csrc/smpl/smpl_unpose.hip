// Unposing (include/cape_hip.h, "SMPL posing, inverse"): from posed vertices in SMPL topology and their pose back to the
// rest body the forward of smpl.hip would have posed into them, and on to the network's normalised displacements.
//
//   cape_smpl_unpose_joints  the rest joints, which the forward regresses from the unknown rest body: one dense 3J x 3J solve
//                            per sample; writes coef and G in cape_smpl_joints' layouts           inverse of demos.py:267-283
//   cape_smpl_unpose_skin    T_v = Mrot_v^-1 (P_v - transl - M_v.t) - basis_v . coef                                 312-326
//   cape_smpl_undress        d = (mask (T - minimal) - mean) / std                                    lib/prep_data.py:74
//
// With W_j the world rotation of joint j, Mrot_v = sum_j w_vj W_j and Jn the rest joints, the forward's skinning translations
// are linear in Jn: G_j.t = sum over m on the path root .. j of D_m Jn_m, D_m = W_parent(m) - W_m (D_0 = I - W_0).  The
// forward regresses Jn from T + shapedirs . betas, and T_v + acc_v = Mrot_v^-1 (P_v - transl - sum_j w_vj G_j.t), so
//   (I + Q L) Jn = c,   Q[a][j] = sum_v jreg[a][v] w_vj Mrot_v^-1,   L[j][m] = D_m if m is on j's path,
//   c = J_regressor . (Mrot^-1 (P - transl)) - jposedirs . pf        (the shape term is on both sides and cancels)
// Q L is assembled as (sum of Q[a][j] over the subtree of m) D_m, walking the regressor's nonzeros only.
#include "smpl_shared.h"

#define UNPOSE_CHUNK 16                    // regressor nonzeros a wave stages per round: [r Mrot^-1 (9) | r Mrot^-1 x (3)]
#define UNPOSE_MAX_N3 (3 * SMPL_MAX_J)
#define UNPOSE_ROWS 8                      // rows a wave eliminates per pass: their loads are in flight together
#ifndef UNPOSE_STAGE_LDS                   // make EXTRA=-DUNPOSE_STAGE_LDS=0 keeps every system in the workspace (the A/B of DESIGN 7g)
#define UNPOSE_STAGE_LDS (43 * 1024)       // the system [3J][3J+1] fp64 is staged in LDS up to this size: J <= 24
#endif

// inverse of a row-major 3x3 by adjugate / determinant; returns the determinant
template <typename T>
__device__ __forceinline__ T inverse3(const T *M, T *Mi) {
    const T c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
    const T det = M[0] * c00 + M[1] * c01 + M[2] * c02;
    const T r = (T)1 / det;
    Mi[0] = c00 * r; Mi[1] = (M[2] * M[7] - M[1] * M[8]) * r; Mi[2] = (M[1] * M[5] - M[2] * M[4]) * r;
    Mi[3] = c01 * r; Mi[4] = (M[0] * M[8] - M[2] * M[6]) * r; Mi[5] = (M[2] * M[3] - M[0] * M[5]) * r;
    Mi[6] = c02 * r; Mi[7] = (M[1] * M[6] - M[0] * M[7]) * r; Mi[8] = (M[0] * M[4] - M[1] * M[3]) * r;
    return det;
}

// ---------------------------------------------------------------------------------------------------------------------
// rest joints: one workgroup of 256 threads per sample.  Rodrigues in fp32 as the forward computes it (coef is the
// forward's); the chain, the assembly and the solve in fp64.  The system [3J][3J+1] (right-hand side in the last column)
// lives in the caller's workspace, or in LDS when STAGED.
template <bool STAGED>
__global__ void __launch_bounds__(256) smpl_unpose_joints_kernel(const float *__restrict__ P, int64_t P_ss, const int32_t *__restrict__ rp,
                                                                 const int32_t *__restrict__ ci, const float *__restrict__ cv,
                                                                 const int32_t *__restrict__ ell_j, const float *__restrict__ ell_w,
                                                                 int32_t W, int32_t V, const float *__restrict__ pose,
                                                                 const float *__restrict__ betas, int32_t B, const float *__restrict__ jpd,
                                                                 const float *__restrict__ transl, SmplTree tree, double *ws,
                                                                 float *__restrict__ coef, float *__restrict__ G,
                                                                 float *__restrict__ rest_joints, float *__restrict__ joints,
                                                                 float *__restrict__ det_min) {
    extern __shared__ double staged[];
    __shared__ float sR[SMPL_MAX_J][9];
    __shared__ double sW[SMPL_MAX_J][9];           // world rotations
    __shared__ double sD[SMPL_MAX_J][9];           // W_parent - W
    __shared__ uint64_t sAnc[SMPL_MAX_J];          // bit m: m is j or an ancestor of j
    __shared__ double sStash[4][UNPOSE_CHUNK][12];
    __shared__ double sX[UNPOSE_MAX_N3];           // the solution: rest joints
    __shared__ int32_t sPiv[UNPOSE_MAX_N3];        // the row that gave column k its pivot
    const int32_t J = tree.J, n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t n3 = 3 * J, ld = n3 + 1;
    double *A = STAGED ? staged : ws + (int64_t)n * n3 * ld;
    const float *Pn = P + n * P_ss;
    const float *pn = pose + (int64_t)n * 3 * J;
    const double t0 = transl ? (double)transl[3 * n] : 0.0, t1 = transl ? (double)transl[3 * n + 1] : 0.0,
                 t2 = transl ? (double)transl[3 * n + 2] : 0.0;

    if (tid < J) {
        float R[9];
        rodrigues(pn[3 * tid], pn[3 * tid + 1], pn[3 * tid + 2], R);
#pragma unroll
        for (int32_t q = 0; q < 9; ++q) sR[tid][q] = R[q];
    }
    if (tid == 0 && det_min) det_min[n] = __builtin_inff();     // cape_smpl_unpose_skin takes the minimum into it
    __syncthreads();
    // coef = [betas | R - I], cape_smpl_joints' layout and values
    const int32_t K = B + 9 * (J - 1);
    float *cn = coef + (int64_t)n * K;
    for (int32_t b = tid; b < B; b += 256) cn[b] = betas[(int64_t)n * B + b];
    if (tid > 0 && tid < J) {
#pragma unroll
        for (int32_t q = 0; q < 9; ++q) cn[B + (tid - 1) * 9 + q] = sR[tid][q] - ((q % 4 == 0) ? 1.f : 0.f);
    }
    // world rotations and ancestor sets, level by level
    if (tid == 0) {
#pragma unroll
        for (int32_t q = 0; q < 9; ++q) {
            sW[0][q] = (double)sR[0][q];
            sD[0][q] = ((q % 4 == 0) ? 1.0 : 0.0) - (double)sR[0][q];
        }
        sAnc[0] = 1ull;
    }
    __syncthreads();
    for (int32_t lvl = 1; lvl <= tree.maxdepth; ++lvl) {
        if (tid < J && tree.depth[tid] == lvl) {
            const int32_t p = tree.parent[tid];
#pragma unroll
            for (int32_t r = 0; r < 3; ++r)
#pragma unroll
                for (int32_t c = 0; c < 3; ++c) {
                    const double w = sW[p][3 * r] * (double)sR[tid][c] + sW[p][3 * r + 1] * (double)sR[tid][3 + c] +
                                     sW[p][3 * r + 2] * (double)sR[tid][6 + c];
                    sW[tid][3 * r + c] = w;
                    sD[tid][3 * r + c] = sW[p][3 * r + c] - w;
                }
            sAnc[tid] = sAnc[p] | (1ull << tid);
        }
        __syncthreads();
    }

    // ---- assembly: wave `wave` takes regressor row a = jb + wave, lane m the 3x3 block (a, m) of I + Q L.  Per round the
    // wave stages r Mrot^-1 and r Mrot^-1 (P - transl) of up to UNPOSE_CHUNK nonzeros, then every lane adds them in entry order
    for (int32_t jb = 0; jb < J; jb += 4) {
        const int32_t a = jb + wave;
        const bool row = a < J;
        const int32_t e0 = row ? rp[a] : 0, e1 = row ? rp[a + 1] : 0;
        int32_t rounds = 0;                              // the same for the four waves: the barriers below are uniform
        for (int32_t w4 = 0; w4 < 4; ++w4)
            if (jb + w4 < J) rounds = max(rounds, (rp[jb + w4 + 1] - rp[jb + w4] + UNPOSE_CHUNK - 1) / UNPOSE_CHUNK);
        double q[9], cs[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int32_t i = 0; i < 9; ++i) q[i] = 0.0;
        for (int32_t rd = 0; rd < rounds; ++rd) {
            const int32_t c0 = e0 + rd * UNPOSE_CHUNK;
            // lane e < UNPOSE_CHUNK owns nonzero c0 + e: one walk over its vertex's skinning weights gives Mrot (own lane) and,
            // handed round the wave, every lane its subtree weight s[e] of that vertex -- no lane waits on another's loads
            const bool mine = lane < UNPOSE_CHUNK && c0 + lane < e1;
            const int32_t v = mine ? ci[c0 + lane] : 0;
            double M[9], s[UNPOSE_CHUNK];
#pragma unroll
            for (int32_t i = 0; i < 9; ++i) M[i] = 0.0;
#pragma unroll
            for (int32_t i = 0; i < UNPOSE_CHUNK; ++i) s[i] = 0.0;
            for (int32_t w0 = 0; w0 < W; w0 += 4) {      // four (joint, weight) pairs per trip to memory; past W: (0, 0.0)
                int32_t jw[4];
                float xw[4];
#pragma unroll
                for (int32_t u = 0; u < 4; ++u) {
                    const bool in = mine && w0 + u < W;
                    jw[u] = in ? ell_j[(w0 + u) * V + v] : 0;
                    xw[u] = in ? ell_w[(w0 + u) * V + v] : 0.f;
                }
#pragma unroll
                for (int32_t u = 0; u < 4; ++u) {
                    const double *g = sW[jw[u]];
#pragma unroll
                    for (int32_t i = 0; i < 9; ++i) M[i] += (double)xw[u] * g[i];
#pragma unroll
                    for (int32_t i = 0; i < UNPOSE_CHUNK; ++i) {
                        const uint64_t anc = sAnc[__shfl(jw[u], i)];
                        const float xi = __shfl(xw[u], i);
                        s[i] += ((anc >> lane) & 1ull) ? (double)xi : 0.0;
                    }
                }
            }
            if (mine) {
                const double r = (double)cv[c0 + lane];
                double Mi[9];
                inverse3(M, Mi);
                const float *p = Pn + 3 * (int64_t)v;
                const double x0 = (double)p[0] - t0, x1 = (double)p[1] - t1, x2 = (double)p[2] - t2;
                double *st = sStash[wave][lane];
#pragma unroll
                for (int32_t i = 0; i < 9; ++i) st[i] = r * Mi[i];
#pragma unroll
                for (int32_t i = 0; i < 3; ++i) st[9 + i] = r * (Mi[3 * i] * x0 + Mi[3 * i + 1] * x1 + Mi[3 * i + 2] * x2);
            }
            __syncthreads();
            const int32_t cnt = e1 - c0;
#pragma unroll
            for (int32_t i = 0; i < UNPOSE_CHUNK; ++i) {
                if (i >= cnt) continue;                  // uniform in the wave
                const double *st = sStash[wave][i];
#pragma unroll
                for (int32_t k = 0; k < 9; ++k) q[k] += s[i] * st[k];
                cs[0] += st[9]; cs[1] += st[10]; cs[2] += st[11];
            }
            __syncthreads();
        }
        if (row) {
            if (lane < J) {
#pragma unroll
                for (int32_t r = 0; r < 3; ++r)
#pragma unroll
                    for (int32_t c = 0; c < 3; ++c)
                        A[(3 * a + r) * ld + 3 * lane + c] = q[3 * r] * sD[lane][c] + q[3 * r + 1] * sD[lane][3 + c] +
                                                             q[3 * r + 2] * sD[lane][6 + c] + ((lane == a && r == c) ? 1.0 : 0.0);
            }
            // - jposedirs . pf: lanes over the pose feature, a fixed butterfly across the wave
            double pj[3] = {0.0, 0.0, 0.0};
            for (int32_t k = lane; k < 9 * (J - 1); k += 64) {
                const int32_t jj = 1 + k / 9, e = k % 9;
                const double pf = (double)(sR[jj][e] - ((e % 4 == 0) ? 1.f : 0.f));
                const float *d = jpd + ((int64_t)k * J + a) * 3;
                pj[0] += pf * (double)d[0]; pj[1] += pf * (double)d[1]; pj[2] += pf * (double)d[2];
            }
#pragma unroll
            for (int32_t o = 32; o > 0; o >>= 1) {
                pj[0] += __shfl_xor(pj[0], o); pj[1] += __shfl_xor(pj[1], o); pj[2] += __shfl_xor(pj[2], o);
            }
            if (lane < 3) A[(3 * a + lane) * ld + n3] = cs[lane] - pj[lane];
        }
    }
    __syncthreads();

    // ---- Gaussian elimination with partial pivoting.  Rows are not exchanged: column k takes its pivot among the rows that
    // have not given one yet (three 64-bit masks, the same in every thread), sPiv[k] remembers it.  Every wave finds the pivot
    // on its own from the same values, so a step has one barrier; loads are unconditional on clamped indices, so that a pass
    // waits once for all of them.  A non-finite entry is never preferred but a row is always chosen, and a zero or non-finite
    // pivot carries on into non-finite results.
    const int32_t wv = __builtin_amdgcn_readfirstlane(wave);
    uint64_t used[3] = {0ull, 0ull, 0ull};
    for (int32_t k = 0; k < n3; ++k) {
        double val = -2.0;
        int32_t idx = 0;
#pragma unroll
        for (int32_t h = 0; h < 3; ++h) {                // rows lane, lane + 64, lane + 128: the lower row keeps a tie
            const int32_t t = lane + 64 * h;
            const double x = fabs(A[min(t, n3 - 1) * ld + k]);
            const bool free_row = t < n3 && !((used[h] >> lane) & 1ull);
            const double cand = free_row ? ((x == x) ? x : -1.0) : -2.0;
            const bool take = cand > val;
            val = take ? cand : val;
            idx = take ? t : idx;
        }
#pragma unroll
        for (int32_t o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(val, o);
            const int32_t oi = __shfl_xor(idx, o);
            const bool take = ov > val || (ov == val && oi < idx);
            val = take ? ov : val;
            idx = take ? oi : idx;
        }
        const int32_t piv = __builtin_amdgcn_readfirstlane(idx);
        const double *prow = A + piv * ld;
        const double rk = 1.0 / prow[k];
        const int32_t c_a = k + 1 + lane, c_b = c_a + 64, c_c = c_b + 64;      // this lane's columns: k+1 .. n3 <= 192
        const int32_t l_a = min(c_a, n3), l_b = min(c_b, n3), l_c = min(c_c, n3);
        const double pa = prow[l_a], pb = prow[l_b], pc = prow[l_c];
        // UNPOSE_ROWS rows per wave and pass
        for (int32_t i0 = wv; i0 < n3; i0 += 4 * UNPOSE_ROWS) {
            double f[UNPOSE_ROWS], xa[UNPOSE_ROWS], xb[UNPOSE_ROWS], xc[UNPOSE_ROWS];
            bool on[UNPOSE_ROWS];
#pragma unroll
            for (int32_t b = 0; b < UNPOSE_ROWS; ++b) {
                const int32_t i = i0 + 4 * b;
                const uint64_t u = i < 64 ? used[0] : (i < 128 ? used[1] : used[2]);
                on[b] = i < n3 && i != piv && !((u >> (i & 63)) & 1ull);
                const double *ar = A + (on[b] ? i : piv) * ld;
                f[b] = ar[k];
                xa[b] = ar[l_a]; xb[b] = ar[l_b]; xc[b] = ar[l_c];
            }
#pragma unroll
            for (int32_t b = 0; b < UNPOSE_ROWS; ++b) {
                if (!on[b]) continue;                    // uniform in the wave
                double *ar = A + (i0 + 4 * b) * ld;
                const double m = f[b] * rk;
                if (c_a <= n3) ar[c_a] = xa[b] - m * pa;
                if (c_b <= n3) ar[c_b] = xb[b] - m * pb;
                if (c_c <= n3) ar[c_c] = xc[b] - m * pc;
            }
        }
        used[0] |= piv < 64 ? 1ull << piv : 0ull;
        used[1] |= (piv >= 64 && piv < 128) ? 1ull << (piv - 64) : 0ull;
        used[2] |= piv >= 128 ? 1ull << (piv - 128) : 0ull;
        if (tid == 0) sPiv[k] = piv;
        __syncthreads();
    }
    // back substitution, column by column
    for (int32_t k = n3 - 1; k >= 0; --k) {
        const int32_t p = sPiv[k];
        if (tid == 0) sX[k] = A[p * ld + n3] / A[p * ld + k];
        __syncthreads();
        if (tid < k) {
            const int32_t pm = sPiv[tid];
            A[pm * ld + n3] -= A[pm * ld + k] * sX[k];
        }
        __syncthreads();
    }

    // ---- G_j = [W_j | sum over j's path of D_m Jn_m], A_j.t = G_j.t + W_j Jn_j
    if (tid < J) {
        double gt[3] = {0.0, 0.0, 0.0};
        const uint64_t anc = sAnc[tid];
        for (int32_t m = 0; m < J; ++m) {
            if (!((anc >> m) & 1ull)) continue;
#pragma unroll
            for (int32_t r = 0; r < 3; ++r)
                gt[r] += sD[m][3 * r] * sX[3 * m] + sD[m][3 * r + 1] * sX[3 * m + 1] + sD[m][3 * r + 2] * sX[3 * m + 2];
        }
        float *g = G + ((int64_t)n * J + tid) * 12;
        const double tr[3] = {t0, t1, t2};
#pragma unroll
        for (int32_t r = 0; r < 3; ++r) {
            const double w0 = sW[tid][3 * r], w1 = sW[tid][3 * r + 1], w2 = sW[tid][3 * r + 2];
            g[4 * r] = (float)w0; g[4 * r + 1] = (float)w1; g[4 * r + 2] = (float)w2;
            g[4 * r + 3] = (float)gt[r];
            const int64_t o = ((int64_t)n * J + tid) * 3 + r;
            if (rest_joints) rest_joints[o] = (float)sX[3 * tid + r];
            if (joints) joints[o] = (float)(gt[r] + w0 * sX[3 * tid] + w1 * sX[3 * tid + 1] + w2 * sX[3 * tid + 2] + tr[r]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// the vertex pass: smpl_skin_kernel's tiling (one thread per vertex, `tile` samples per workgroup of 64 or 256 threads, coef
// [K][tile] and G [tile][J][12] in LDS, the basis streamed once per tile).  M is blended in fp32 in the forward's order, so
// it is the forward's M bit for bit; its inverse and the product with P - transl - M.t are fp64, rounded once; the blend
// offset is subtracted in fp32 (widening the 48 accumulators costs 50 registers and half the waves per SIMD).
__global__ void __launch_bounds__(256) smpl_unpose_skin_kernel(const float *__restrict__ P, int64_t P_ss, const float *__restrict__ basis,
                                                               int32_t K, const float *__restrict__ coef, const float *__restrict__ G,
                                                               const int32_t *__restrict__ ell_j, const float *__restrict__ ell_w,
                                                               int32_t W, const float *__restrict__ transl, int32_t J, int32_t V,
                                                               int32_t N, int32_t tile, float *__restrict__ out, int64_t out_ss,
                                                               float *__restrict__ det_min) {
    extern __shared__ float lds[];
    float *sC = lds;                              // [K][tile]
    float *sG = lds + ((K * tile + 3) & ~3);      // [tile][J][12], 16-byte aligned
    const int32_t n0 = blockIdx.y * tile, ns = min(tile, N - n0);
    const int32_t nt = blockDim.x;
    for (int32_t i = threadIdx.x; i < K * ns; i += nt) {
        const int32_t s = i / K, k = i - s * K;
        sC[k * tile + s] = coef[(int64_t)(n0 + s) * K + k];
    }
    for (int32_t i = threadIdx.x; i < 12 * J * ns; i += nt) sG[i] = G[(int64_t)n0 * 12 * J + i];
    __syncthreads();
    // every lane stays for the wave minimum: one past the last vertex reads vertex V-1 and stores nothing
    const int32_t v = blockIdx.x * nt + threadIdx.x;
    const bool live = v < V;
    const int32_t vc = live ? v : V - 1;

    float acc[SMPL_TILE][3];
#pragma unroll
    for (int32_t s = 0; s < SMPL_TILE; ++s) acc[s][0] = acc[s][1] = acc[s][2] = 0.f;
#pragma unroll 2
    for (int32_t k = 0; k < K; ++k) {
        const float bx = basis[(3 * k) * V + vc], by = basis[(3 * k + 1) * V + vc], bz = basis[(3 * k + 2) * V + vc];
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
        if (s >= ns) continue;              // ns is uniform: a scalar branch
        const int64_t n = n0 + s;
        float M[12];
#pragma unroll
        for (int32_t q = 0; q < 12; ++q) M[q] = 0.f;
        for (int32_t w = 0; w < W; ++w) {
            const float a = ell_w[w * V + vc];
            const float4 *g = reinterpret_cast<const float4 *>(sG + (s * J + ell_j[w * V + vc]) * 12);
            const float4 g0 = g[0], g1 = g[1], g2 = g[2];
            M[0] += a * g0.x; M[1] += a * g0.y; M[2] += a * g0.z;  M[3] += a * g0.w;
            M[4] += a * g1.x; M[5] += a * g1.y; M[6] += a * g1.z;  M[7] += a * g1.w;
            M[8] += a * g2.x; M[9] += a * g2.y; M[10] += a * g2.z; M[11] += a * g2.w;
        }
        const double Mr[9] = {(double)M[0], (double)M[1], (double)M[2], (double)M[4], (double)M[5], (double)M[6],
                              (double)M[8], (double)M[9], (double)M[10]};
        double Mi[9];
        const double det = inverse3(Mr, Mi);
        const float *p = P + n * P_ss + 3 * vc;
        double x[3];
#pragma unroll
        for (int32_t r = 0; r < 3; ++r) x[r] = (double)p[r] - (transl ? (double)transl[3 * n + r] : 0.0) - (double)M[4 * r + 3];
        if (live) {
            float *o = out + n * out_ss + 3 * v;
#pragma unroll
            for (int32_t r = 0; r < 3; ++r)
                o[r] = (float)(Mi[3 * r] * x[0] + Mi[3 * r + 1] * x[1] + Mi[3 * r + 2] * x[2]) - acc[s][r];
        }
        if (det_min) {
            // |det| >= 0: its bit pattern orders as the value does, and a NaN's lies above +inf's and is never taken
            uint32_t d = live ? __float_as_uint(fabsf((float)det)) : 0x7f800000u;
#pragma unroll
            for (int32_t o = 32; o > 0; o >>= 1) d = min(d, (uint32_t)__shfl_xor((int32_t)d, o));
            if ((threadIdx.x & 63) == 0) atomicMin(reinterpret_cast<uint32_t *>(det_min) + n, d);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// undress: one thread per scalar of a sample's [V, 3] block
__global__ void __launch_bounds__(256) smpl_undress_kernel(const float *__restrict__ T, int64_t T_ss, const float *__restrict__ mean,
                                                           const float *__restrict__ std_, const float *__restrict__ mask,
                                                           const float *__restrict__ minimal, float *__restrict__ d, int64_t d_ss,
                                                           int32_t V3) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V3) return;
    const int64_t n = blockIdx.y;
    const float x = T[n * T_ss + i] - minimal[i];
    d[n * d_ss + i] = ((mask ? mask[i / 3] * x : x) - mean[i]) / std_[i];
}

// ---------------------------------------------------------------------------------------------------------------------
extern "C" int64_t cape_smpl_unpose_workspace_bytes(int32_t J, int32_t N) {
    if (J < 1 || J > SMPL_MAX_J || N < 1) return CAPE_EINVAL;
    return 8LL * N * (3 * J) * (3 * J + 1);
}

extern "C" int cape_smpl_unpose_joints(const float *posed, int64_t posed_sample_stride, const int32_t *jreg_rowptr,
                                       const int32_t *jreg_colidx, const float *jreg_vals, const int32_t *ell_joint,
                                       const float *ell_weight, int32_t ell_width, const float *pose, const float *betas,
                                       int32_t B, const float *jposedirs, const float *transl, const int32_t *parents, int32_t J,
                                       int32_t V, int32_t N, void *workspace, int64_t workspace_bytes, float *coef, float *G,
                                       float *rest_joints, float *joints, float *det_min, void *stream) {
    SmplTree tree;
    const int rc = smpl_tree(parents, J, &tree);
    if (rc) return rc;
    if (!posed || !jreg_rowptr || !jreg_colidx || !jreg_vals || !ell_joint || !ell_weight || !pose || !coef || !G || !workspace)
        return CAPE_EINVAL;
    if (J > 1 && !jposedirs) return CAPE_EINVAL;
    if (B < 0 || (B > 0 && !betas)) return CAPE_EINVAL;
    if (N < 1 || V < 1 || V > (1 << 29) || ell_width < 1 || ell_width > J || posed_sample_stride < 3LL * V) return CAPE_EINVAL;
    if ((int64_t)ell_width * V >= (1LL << 31)) return CAPE_EINVAL;                                   // 32-bit element index
    if (((uintptr_t)workspace & 7) || workspace_bytes < cape_smpl_unpose_workspace_bytes(J, N)) return CAPE_EINVAL;
    const size_t sys = 8 * (size_t)(3 * J) * (3 * J + 1);
    if (sys <= UNPOSE_STAGE_LDS)
        smpl_unpose_joints_kernel<true><<<N, 256, sys, (hipStream_t)stream>>>(posed, posed_sample_stride, jreg_rowptr, jreg_colidx,
            jreg_vals, ell_joint, ell_weight, ell_width, V, pose, betas, B, jposedirs, transl, tree, (double *)workspace, coef, G,
            rest_joints, joints, det_min);
    else
        smpl_unpose_joints_kernel<false><<<N, 256, 0, (hipStream_t)stream>>>(posed, posed_sample_stride, jreg_rowptr, jreg_colidx,
            jreg_vals, ell_joint, ell_weight, ell_width, V, pose, betas, B, jposedirs, transl, tree, (double *)workspace, coef, G,
            rest_joints, joints, det_min);
    return launch_status();
}

extern "C" int cape_smpl_unpose_skin(const float *posed, int64_t posed_sample_stride, const float *basis, int32_t K,
                                     const float *coef, const float *G, const int32_t *ell_joint, const float *ell_weight,
                                     int32_t ell_width, const float *transl, int32_t J, int32_t V, int32_t N, float *out,
                                     int64_t out_sample_stride, float *det_min, void *stream) {
    const int tile = cape_smpl_skin_tile(K, J);
    if (tile < 0) return tile;
    if (!posed || (K > 0 && (!basis || !coef)) || !G || !ell_joint || !ell_weight || !out) return CAPE_EINVAL;
    if (N < 1 || V < 1 || ell_width < 1 || ell_width > J) return CAPE_EINVAL;
    if (3LL * K * V >= (1LL << 31) || (int64_t)ell_width * V >= (1LL << 31)) return CAPE_EINVAL;   // 32-bit element index
    if (posed_sample_stride < 3LL * V || out_sample_stride < 3LL * V) return CAPE_EINVAL;
    const int32_t tiles = (N + tile - 1) / tile;
    if (tiles > 65535) return CAPE_EINVAL;
    // cape_smpl_skin's rule: 256-thread workgroups once they fill the chip, below that one wave each
    const int32_t threads = (int64_t)tiles * ((V + 255) / 256) >= 256 ? 256 : 64;
    dim3 grid((V + threads - 1) / threads, tiles);
    const size_t lds = 4 * (size_t)(((K * tile + 3) & ~3) + 12 * J * tile);
    smpl_unpose_skin_kernel<<<grid, threads, lds, (hipStream_t)stream>>>(posed, posed_sample_stride, basis, K, coef, G, ell_joint,
                                                                     ell_weight, ell_width, transl, J, V, N, tile, out,
                                                                     out_sample_stride, det_min);
    return launch_status();
}

extern "C" int cape_smpl_undress(const float *T, int64_t T_sample_stride, const float *mean, const float *std_, const float *mask,
                                 const float *minimal, float *disp, int64_t disp_sample_stride, int32_t N, int32_t V,
                                 void *stream) {
    if (!T || !mean || !std_ || !minimal || !disp) return CAPE_EINVAL;
    if (N < 1 || N > 65535 || V < 1 || V > (1 << 29)) return CAPE_EINVAL;
    if (T_sample_stride < 3LL * V || disp_sample_stride < 3LL * V) return CAPE_EINVAL;
    dim3 grid((3 * V + 255) / 256, N);
    smpl_undress_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(T, T_sample_stride, mean, std_, mask, minimal, disp,
                                                                disp_sample_stride, 3 * V);
    return launch_status();
}
