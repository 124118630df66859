// Backward of SMPL posing (include/cape_hip.h, "SMPL posing, backward"): given the gradients on the posed vertices and / or
// the posed joints, the gradients on the rest body, the pose, the shape coefficients and the translation.
//
//   cape_smpl_skin_bwd    the vertex pass: q = M_v.rot^T gV_v, and per workgroup the partial sums over its vertices of
//                         gcoef_k = basis[k,:,v] . q_v,  dG_j = W_vj gV_v (x) [v_p; 1]  and  gV_v
//   cape_smpl_joints_bwd  sums the partials (fp64), recomputes joints / rotations / chain as the forward ran them, runs the
//                         chain and Rodrigues' formula backwards (fp64): dpose, dbetas, dtransl, dJn
//   cape_smpl_jreg_bwd    dT = q + J_regressor^T dJn, summed over the samples when they share one rest body
//   cape_smpl_dress_bwd   d_disp = mask * std * g
//   cape_smpl_weighted_l2 per-sample sum_v w_v |pred_v - target_v|^2 / sum_v w_v and its gradient (the data term of fit_posed)
//
// No atomics: every sum has a fixed order, results are bitwise repeatable.
#include "smpl_shared.h"

#define SMPL_BWD_KC 16                        // coefficient planes per cross-wave exchange
#define SMPL_BWD_XCH (4 * 16 * SMPL_BWD_KC)   // exchange buffer: [wave][16 rows][16 samples] floats

// x[s], s < 16, summed over the 64 lanes of the wave: every lane gets the total of x[(lane >> 2) & 15].  Four halving
// exchanges (each lane gives away the half of its values that its partner keeps) and two plain butterfly steps: 17 cross-lane
// moves instead of 96, always the same tree.
__device__ __forceinline__ float wave_sum16(const float (&x)[16]) {
    const int32_t lane = threadIdx.x & 63;
    float a[8], b[4], c[2];
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8, h2 = lane & 4;
#pragma unroll
    for (int32_t i = 0; i < 8; ++i) a[i] = (h5 ? x[i + 8] : x[i]) + __shfl_xor(h5 ? x[i] : x[i + 8], 32);
#pragma unroll
    for (int32_t i = 0; i < 4; ++i) b[i] = (h4 ? a[i + 4] : a[i]) + __shfl_xor(h4 ? a[i] : a[i + 4], 16);
#pragma unroll
    for (int32_t i = 0; i < 2; ++i) c[i] = (h3 ? b[i + 2] : b[i]) + __shfl_xor(h3 ? b[i] : b[i + 2], 8);
    float d = (h2 ? c[1] : c[0]) + __shfl_xor(h2 ? c[0] : c[1], 4);
    d += __shfl_xor(d, 2);
    d += __shfl_xor(d, 1);
    return d;
}

// the waves' entries of the exchange buffer in a fixed pairwise order
__device__ __forceinline__ float xch_sum(const float *sX, int32_t nw, int32_t i) {
    return nw == 4 ? (sX[i] + sX[256 + i]) + (sX[512 + i] + sX[768 + i]) : sX[i];
}

// ---------------------------------------------------------------------------------------------------------------------
// the vertex pass: smpl_skin_kernel's tiling (one thread per vertex, `tile` samples per workgroup of 64 or 256 threads, coef
// [K][tile] and G [tile][J][12] in LDS, the basis streamed once per tile).  Record of (sample, workgroup) in `part`:
// [gcoef K | dG J x 12 | sum gV 3]
template <bool COEF>
__global__ void __launch_bounds__(256) smpl_skin_bwd_kernel(const float *__restrict__ T, int64_t T_ss, const float *__restrict__ basis,
                                                            int32_t K, const float *__restrict__ coef, const float *__restrict__ G,
                                                            const int32_t *__restrict__ ell_j, const float *__restrict__ ell_w,
                                                            int32_t W, const float *__restrict__ gV, int64_t gV_ss, int32_t J,
                                                            int32_t V, int32_t N, int32_t tile, float *__restrict__ q_out,
                                                            int64_t q_ss, float *__restrict__ part) {
    extern __shared__ float lds[];
    float *sC = lds;                              // [K][tile]
    float *sG = lds + ((K * tile + 3) & ~3);      // [tile][J][12], 16-byte aligned
    float *sX = sG + 12 * J * tile;               // [wave][16][16]
    const int32_t n0 = blockIdx.y * tile, ns = min(tile, N - n0);
    const int32_t nt = blockDim.x, nw = nt >> 6, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t P = K + 12 * J + 3, nblk = gridDim.x;
    for (int32_t i = tid; i < K * ns; i += nt) {
        const int32_t s = i / K, k = i - s * K;
        sC[k * tile + s] = coef[(int64_t)(n0 + s) * K + k];
    }
    for (int32_t i = tid; i < 12 * J * ns; i += nt) sG[i] = G[(int64_t)n0 * 12 * J + i];
    __syncthreads();
    // every lane stays for the reductions: one past the last vertex reads vertex V-1 and carries a zero gradient
    const int32_t v = blockIdx.x * nt + tid;
    const bool live = v < V;
    const int32_t vc = live ? v : V - 1;
    const bool slot = (lane & 3) == 0;
    const int32_t ls = lane >> 2;

    float q[SMPL_TILE][3], acc[SMPL_TILE][3];
#pragma unroll
    for (int32_t s = 0; s < SMPL_TILE; ++s) {
        acc[s][0] = acc[s][1] = acc[s][2] = 0.f;
        q[s][0] = q[s][1] = q[s][2] = 0.f;
        if (s >= ns) continue;
        const int64_t n = n0 + s;
        float M[9];
#pragma unroll
        for (int32_t i = 0; i < 9; ++i) M[i] = 0.f;
        for (int32_t w = 0; w < W; ++w) {          // the forward's M.rot: the nonzero weights in increasing joint order
            const float a = ell_w[w * V + vc];
            const float4 *g = reinterpret_cast<const float4 *>(sG + (s * J + ell_j[w * V + vc]) * 12);
            const float4 g0 = g[0], g1 = g[1], g2 = g[2];
            M[0] += a * g0.x; M[1] += a * g0.y; M[2] += a * g0.z;
            M[3] += a * g1.x; M[4] += a * g1.y; M[5] += a * g1.z;
            M[6] += a * g2.x; M[7] += a * g2.y; M[8] += a * g2.z;
        }
        const float *gp = gV + n * gV_ss + 3 * vc;
        const float gx = live ? gp[0] : 0.f, gy = live ? gp[1] : 0.f, gz = live ? gp[2] : 0.f;
#pragma unroll
        for (int32_t c = 0; c < 3; ++c) q[s][c] = M[c] * gx + M[3 + c] * gy + M[6 + c] * gz;
        if (q_out && live) {
            float *o = q_out + n * q_ss + 3 * v;
            o[0] = q[s][0]; o[1] = q[s][1]; o[2] = q[s][2];
        }
    }
    // one walk over the basis: v_p - T for the tile's samples, and each plane's dot with q summed over the workgroup
    for (int32_t k0 = 0; k0 < K; k0 += SMPL_BWD_KC) {
        const int32_t kn = min(SMPL_BWD_KC, K - k0);
        for (int32_t kk = 0; kk < kn; ++kk) {
            const int32_t k = k0 + kk;
            const float bx = basis[(3 * k) * V + vc], by = basis[(3 * k + 1) * V + vc], bz = basis[(3 * k + 2) * V + vc];
            const float *c = sC + k * tile;
            float x[SMPL_TILE];
#pragma unroll
            for (int32_t s = 0; s < SMPL_TILE; ++s) {
                x[s] = 0.f;
                if (s < ns) {
                    const float w = c[s];
                    acc[s][0] += w * bx; acc[s][1] += w * by; acc[s][2] += w * bz;
                    if (COEF) x[s] = bx * q[s][0] + by * q[s][1] + bz * q[s][2];
                }
            }
            if (COEF) {
                const float r = wave_sum16(x);
                if (slot) sX[wave * 256 + kk * 16 + ls] = r;
            }
        }
        if (COEF) {
            __syncthreads();
            for (int32_t i = tid; i < 256; i += nt) {       // sample-major: 16 consecutive words of one record per sample
                const int32_t s = i >> 4, kk = i & 15;
                if (s < ns && kk < kn) part[((int64_t)(n0 + s) * nblk + blockIdx.x) * P + k0 + kk] = xch_sum(sX, nw, kk * 16 + s);
            }
            __syncthreads();
        }
    }
    // v_p, and the gradient again (q is done)
    float g[SMPL_TILE][3];
#pragma unroll
    for (int32_t s = 0; s < SMPL_TILE; ++s) {
        g[s][0] = g[s][1] = g[s][2] = 0.f;
        if (s >= ns) continue;
        const int64_t n = n0 + s;
        const float *t = T + n * T_ss + 3 * vc, *gp = gV + n * gV_ss + 3 * vc;
        acc[s][0] += t[0]; acc[s][1] += t[1]; acc[s][2] += t[2];
        if (live) { g[s][0] = gp[0]; g[s][1] = gp[1]; g[s][2] = gp[2]; }
    }
    // dG_j = sum_v W_vj gV_v (x) [v_p; 1]: joint by joint; a wave none of whose vertices hangs on the joint contributes zeros
    for (int32_t j = 0; j < J; ++j) {
        float a = 0.f;
        for (int32_t w = 0; w < W; ++w) a += (ell_j[w * V + vc] == j) ? ell_w[w * V + vc] : 0.f;
        const bool any = __ballot(a != 0.f) != 0;
#pragma unroll
        for (int32_t c = 0; c < 12; ++c) {
            float r = 0.f;
            if (any) {
                float x[SMPL_TILE];
#pragma unroll
                for (int32_t s = 0; s < SMPL_TILE; ++s) x[s] = (c & 3) == 3 ? a * g[s][c >> 2] : a * g[s][c >> 2] * acc[s][(c & 3) % 3];
                r = wave_sum16(x);
            }
            if (slot) sX[wave * 256 + c * 16 + ls] = r;
        }
        __syncthreads();
        for (int32_t i = tid; i < 12 * 16; i += nt) {
            const int32_t s = i / 12, c = i - 12 * s;
            if (s < ns) part[((int64_t)(n0 + s) * nblk + blockIdx.x) * P + K + 12 * j + c] = xch_sum(sX, nw, c * 16 + s);
        }
        __syncthreads();
    }
#pragma unroll
    for (int32_t c = 0; c < 3; ++c) {
        float x[SMPL_TILE];
#pragma unroll
        for (int32_t s = 0; s < SMPL_TILE; ++s) x[s] = g[s][c];
        const float r = wave_sum16(x);
        if (slot) sX[wave * 256 + c * 16 + ls] = r;
    }
    __syncthreads();
    for (int32_t i = tid; i < 3 * 16; i += nt) {
        const int32_t s = i / 3, c = i - 3 * s;
        if (s < ns) part[((int64_t)(n0 + s) * nblk + blockIdx.x) * P + K + 12 * J + c] = xch_sum(sX, nw, c * 16 + s);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// joints + chain backward: one workgroup of 256 threads per sample.  The forward values in fp32 as the forward computed them,
// every gradient in fp64 (at most 64 joints: the cost is nothing), rounded once on the way out.
__global__ void __launch_bounds__(256) smpl_joints_bwd_kernel(const float *__restrict__ T, int64_t T_ss, const int32_t *__restrict__ rp,
                                                              const int32_t *__restrict__ ci, const float *__restrict__ cv,
                                                              const float *__restrict__ pose, const float *__restrict__ betas,
                                                              int32_t B, const float *__restrict__ jsd, SmplTree tree,
                                                              const float *__restrict__ gJ, const float *__restrict__ part,
                                                              int32_t nblk, int32_t coef_valid, float *__restrict__ dpose, float *__restrict__ dbetas,
                                                              float *__restrict__ dtransl, float *__restrict__ dJn) {
    __shared__ float sJ[SMPL_MAX_J][3];
    __shared__ float sR[SMPL_MAX_J][9];
    __shared__ float sA[SMPL_MAX_J][12];
    __shared__ double sdG[SMPL_MAX_J][12];      // the summed partials, then dA_j = [rot | t] (3 rows of 4)
    __shared__ double sUp[SMPL_MAX_J][12];      // what joint j hands to its parent's dA
    __shared__ double sU[SMPL_MAX_J][3];        // A_p.rot^T dA_j.t
    __shared__ double sdJ[SMPL_MAX_J][3];
    __shared__ double sdR[SMPL_MAX_J][9];
    __shared__ double sgs[3];
    const int32_t J = tree.J, n = blockIdx.x, tid = threadIdx.x;
    const int32_t K = B + 9 * (J - 1), P = K + 12 * J + 3;
    const float *pn = pose + (int64_t)n * 3 * J;
    smpl_chain(T + n * T_ss, rp, ci, cv, pn, betas + (int64_t)n * B, B, jsd, tree, sJ, sR, sA);
    const float *pw = part ? part + (int64_t)n * nblk * P : nullptr;
    const float *pc = coef_valid ? pw : nullptr;      // the records' gcoef words are written only when asked for
    // the workgroup partials of the vertex pass: at most a few hundred per quantity, summed in fp64
    for (int32_t i = tid; i < 12 * J + 3; i += 256) {
        double a = 0.0;
        if (pw)
            for (int32_t b = 0; b < nblk; ++b) a += (double)pw[(int64_t)b * P + K + i];
        if (i < 12 * J) sdG[i / 12][i % 12] = a;
        else sgs[i - 12 * J] = a;
    }
    for (int32_t i = tid; i < 9 * J; i += 256) {
        double a = 0.0;
        if (pc && i >= 9)                           // gcoef's pose rows: the pose feature's direct path into v_p
            for (int32_t b = 0; b < nblk; ++b) a += (double)pw[(int64_t)b * P + B + (i - 9)];
        sdR[i / 9][i % 9] = a;
    }
    __syncthreads();
    if (tid < J) {
        double gt[3];
#pragma unroll
        for (int32_t r = 0; r < 3; ++r) gt[r] = sdG[tid][4 * r + 3];
#pragma unroll
        for (int32_t r = 0; r < 3; ++r) {
#pragma unroll
            for (int32_t c = 0; c < 3; ++c) sdG[tid][4 * r + c] -= gt[r] * (double)sJ[tid][c];          // dA.rot = dG.rot - dG.t (x) Jn
            sdG[tid][4 * r + 3] = gt[r] + (gJ ? (double)gJ[((int64_t)n * J + tid) * 3 + r] : 0.0);      // dA.t = dG.t + gJ
        }
#pragma unroll
        for (int32_t c = 0; c < 3; ++c)                                                                   // dJn = -A.rot^T dG.t
            sdJ[tid][c] = -((double)sA[tid][c] * gt[0] + (double)sA[tid][4 + c] * gt[1] + (double)sA[tid][8 + c] * gt[2]);
    }
    __syncthreads();
    // leaves to root: a level's joints finish, then their parents take them in increasing joint order
    for (int32_t lvl = tree.maxdepth; lvl >= 1; --lvl) {
        if (tid < J && tree.depth[tid] == lvl) {
            const int32_t p = tree.parent[tid];
            double d[12], Rp[9];
#pragma unroll
            for (int32_t i = 0; i < 12; ++i) d[i] = sdG[tid][i];
#pragma unroll
            for (int32_t r = 0; r < 3; ++r)
#pragma unroll
                for (int32_t c = 0; c < 3; ++c) Rp[3 * r + c] = (double)sA[p][4 * r + c];
#pragma unroll
            for (int32_t a = 0; a < 3; ++a)
#pragma unroll
                for (int32_t b = 0; b < 3; ++b)                                                       // dR_j = A_p.rot^T dA_j.rot
                    sdR[tid][3 * a + b] += Rp[a] * d[b] + Rp[3 + a] * d[4 + b] + Rp[6 + a] * d[8 + b];
#pragma unroll
            for (int32_t r = 0; r < 3; ++r) {
#pragma unroll
                for (int32_t c = 0; c < 3; ++c)                              // dA_j.rot R_j^T + dA_j.t (x) (Jn_j - Jn_p)
                    sUp[tid][4 * r + c] = d[4 * r] * (double)sR[tid][3 * c] + d[4 * r + 1] * (double)sR[tid][3 * c + 1] +
                                          d[4 * r + 2] * (double)sR[tid][3 * c + 2] +
                                          d[4 * r + 3] * ((double)sJ[tid][c] - (double)sJ[p][c]);
                sUp[tid][4 * r + 3] = d[4 * r + 3];
            }
#pragma unroll
            for (int32_t c = 0; c < 3; ++c) {
                const double u = Rp[c] * d[3] + Rp[3 + c] * d[7] + Rp[6 + c] * d[11];
                sU[tid][c] = u;
                sdJ[tid][c] += u;
            }
        }
        __syncthreads();
        if (tid < J && tree.depth[tid] == lvl - 1) {
            for (int32_t j = tid + 1; j < J; ++j) {
                if (tree.parent[j] != tid) continue;
#pragma unroll
                for (int32_t i = 0; i < 12; ++i) sdG[tid][i] += sUp[j][i];
#pragma unroll
                for (int32_t c = 0; c < 3; ++c) sdJ[tid][c] -= sU[j][c];
            }
        }
        __syncthreads();
    }
    if (tid < 3) sdJ[0][tid] += sdG[0][4 * tid + 3];        // A_0 = [R_0 | Jn_0]
    if (tid < 9) sdR[0][tid] += sdG[0][4 * (tid / 3) + tid % 3];
    __syncthreads();
    // Rodrigues backward: R = I + s K + c (r r^T - t2 I), s and c functions of t2 = |r|^2.  With D = dR:
    //   dr = s a + c ((D + D^T) r - 2 tr(D) r) + 2 (s' r.a + c' (r^T D r - t2 tr D)) r,   a = (D21 - D12, D02 - D20, D10 - D01)
    // below t2 = 1e-6 the forward's series: s' = -1/6, c' = -1/24 (at r = 0: dr = a, the generators); above it
    // s' = (cos t - s) / (2 t2), c' = (s / 2 - c) / t2
    if (dpose && tid < J) {
        const float fx = pn[3 * tid], fy = pn[3 * tid + 1], fz = pn[3 * tid + 2];
        const double r[3] = {(double)fx, (double)fy, (double)fz};
        const double t2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
        double s, c, s1, c1;
        if (smpl_small_angle(smpl_theta2(fx, fy, fz))) {    // the forward's own test (smpl_shared.h)
            s = 1.0 - t2 * (1.0 / 6.0);
            c = 0.5 - t2 * (1.0 / 24.0);
            s1 = -1.0 / 6.0;
            c1 = -1.0 / 24.0;
        } else {
            const double t = sqrt(t2), h = sin(0.5 * t) / t;
            s = sin(t) / t;
            c = 2.0 * h * h;
            s1 = (cos(t) - s) / (2.0 * t2);
            c1 = (0.5 * s - c) / t2;
        }
        double D[9];
#pragma unroll
        for (int32_t i = 0; i < 9; ++i) D[i] = sdR[tid][i];
        const double a[3] = {D[7] - D[5], D[2] - D[6], D[3] - D[1]};
        const double tr = D[0] + D[4] + D[8];
        double Dr[3], DTr[3];
#pragma unroll
        for (int32_t i = 0; i < 3; ++i) {
            Dr[i] = D[3 * i] * r[0] + D[3 * i + 1] * r[1] + D[3 * i + 2] * r[2];
            DTr[i] = D[i] * r[0] + D[3 + i] * r[1] + D[6 + i] * r[2];
        }
        const double ra = r[0] * a[0] + r[1] * a[1] + r[2] * a[2];
        const double rDr = r[0] * Dr[0] + r[1] * Dr[1] + r[2] * Dr[2];
        const double dt2 = s1 * ra + c1 * (rDr - t2 * tr);
#pragma unroll
        for (int32_t i = 0; i < 3; ++i)
            dpose[(int64_t)n * 3 * J + 3 * tid + i] = (float)(s * a[i] + c * (Dr[i] + DTr[i] - 2.0 * tr * r[i]) + 2.0 * dt2 * r[i]);
    }
    if (dJn && tid < 3 * J) dJn[(int64_t)n * 3 * J + tid] = (float)sdJ[tid / 3][tid % 3];
    if (dbetas) {
        for (int32_t b = tid; b < B; b += 256) {
            double a = 0.0;
            if (pc)
                for (int32_t k = 0; k < nblk; ++k) a += (double)pw[(int64_t)k * P + b];
            for (int32_t i = 0; i < 3 * J; ++i) a += (double)jsd[b * 3 * J + i] * sdJ[i / 3][i % 3];
            dbetas[(int64_t)n * B + b] = (float)a;
        }
    }
    if (dtransl && tid < 3) {
        double a = sgs[tid];
        if (gJ)
            for (int32_t j = 0; j < J; ++j) a += (double)gJ[((int64_t)n * J + j) * 3 + tid];
        dtransl[3 * (int64_t)n + tid] = (float)a;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// dT = q + J_regressor^T dJn: one thread per scalar, a gather through the regressor's columns (CSC); with `shared` the
// samples are summed as well, in fp64 and in sample order
__global__ void __launch_bounds__(256) smpl_jreg_bwd_kernel(const float *__restrict__ q, int64_t q_ss, const int32_t *__restrict__ cp,
                                                            const int32_t *__restrict__ ri, const float *__restrict__ va,
                                                            const float *__restrict__ dJn, int32_t J, int32_t V3, int32_t N,
                                                            int32_t shared, float *__restrict__ dT, int64_t dT_ss) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V3) return;
    const int32_t v = i / 3, c = i - 3 * v, e0 = cp[v], e1 = cp[v + 1];
    if (!shared) {
        const int64_t n = blockIdx.y;
        float a = q ? q[n * q_ss + i] : 0.f;
        for (int32_t e = e0; e < e1; ++e) a += va[e] * dJn[(n * J + ri[e]) * 3 + c];
        dT[n * dT_ss + i] = a;
        return;
    }
    double t = 0.0;
    for (int64_t n = 0; n < N; ++n) {
        float a = q ? q[n * q_ss + i] : 0.f;
        for (int32_t e = e0; e < e1; ++e) a += va[e] * dJn[(n * J + ri[e]) * 3 + c];
        t += (double)a;
    }
    dT[i] = (float)t;
}

__global__ void __launch_bounds__(256) smpl_dress_bwd_kernel(const float *__restrict__ g, int64_t g_ss, const float *__restrict__ std_,
                                                             const float *__restrict__ mask, float *__restrict__ dd, int64_t dd_ss,
                                                             int32_t V3) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V3) return;
    const int64_t n = blockIdx.y;
    dd[n * dd_ss + i] = mask[i / 3] * std_[i] * g[n * g_ss + i];
}

// loss[n] = inv_wsum sum_v w_v |pred - target|^2, grad = 2 inv_wsum w_v (pred - target): one workgroup per sample, fp64 sums
__global__ void __launch_bounds__(256) smpl_weighted_l2_kernel(const float *__restrict__ pred, int64_t p_ss, const float *__restrict__ target,
                                                               int64_t t_ss, const float *__restrict__ w, float inv_wsum, int32_t V,
                                                               float *__restrict__ loss, float *__restrict__ grad, int64_t g_ss) {
    __shared__ double red[256];
    const int64_t n = blockIdx.x;
    double a = 0.0;
    for (int32_t v = threadIdx.x; v < V; v += 256) {
        const float wv = w[v];
        float d2 = 0.f;
#pragma unroll
        for (int32_t c = 0; c < 3; ++c) {
            const float d = pred[n * p_ss + 3 * v + c] - target[n * t_ss + 3 * v + c];
            d2 += d * d;
            if (grad) grad[n * g_ss + 3 * v + c] = 2.f * inv_wsum * wv * d;
        }
        a += (double)wv * (double)d2;
    }
    red[threadIdx.x] = a;
    __syncthreads();
    for (int32_t o = 128; o > 0; o >>= 1) {
        if ((int32_t)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[n] = (float)(red[0] * (double)inv_wsum);
}

// ---------------------------------------------------------------------------------------------------------------------
static int bwd_tile(int32_t K, int32_t J) {
    if (K < 0 || J < 1 || J > SMPL_MAX_J) return CAPE_EINVAL;
    const int64_t per_sample = 4LL * K + 48LL * J;
    const int64_t t = (SMPL_SKIN_LDS - 16 - 4 * SMPL_BWD_XCH) / per_sample;
    return t < 1 ? CAPE_EINVAL : (int)(t < SMPL_TILE ? t : SMPL_TILE);
}

// cape_smpl_skin's rule: 256-thread workgroups once they fill the chip, below that one wave each
static int32_t bwd_threads(int64_t tiles, int32_t V) { return tiles * ((V + 255) / 256) >= 256 ? 256 : 64; }

extern "C" int cape_smpl_skin_bwd_plan(int32_t K, int32_t J, int32_t V, int32_t N, int32_t *plan) {
    const int tile = bwd_tile(K, J);
    if (tile < 0) return tile;
    if (!plan || V < 1 || V > (1 << 29) || N < 1) return CAPE_EINVAL;
    const int64_t tiles = (N + tile - 1) / tile;
    if (tiles > 65535) return CAPE_EINVAL;
    const int32_t threads = bwd_threads(tiles, V);
    plan[0] = tile;
    plan[1] = (V + threads - 1) / threads;
    plan[2] = K + 12 * J + 3;
    return CAPE_OK;
}

extern "C" int64_t cape_smpl_skin_bwd_workspace_bytes(int32_t K, int32_t J, int32_t V, int32_t N) {
    int32_t plan[3];
    const int rc = cape_smpl_skin_bwd_plan(K, J, V, N, plan);
    return rc ? rc : 4LL * N * plan[1] * plan[2];
}

extern "C" int cape_smpl_skin_bwd(const float *T, int64_t T_sample_stride, const float *basis, int32_t K, const float *coef,
                                  const float *G, const int32_t *ell_joint, const float *ell_weight, int32_t ell_width,
                                  const float *gV, int64_t gV_sample_stride, int32_t J, int32_t V, int32_t N, int32_t need_coef,
                                  float *q, int64_t q_sample_stride, void *workspace, int64_t workspace_bytes, void *stream) {
    int32_t plan[3];
    const int rc = cape_smpl_skin_bwd_plan(K, J, V, N, plan);
    if (rc) return rc;
    if (!T || (K > 0 && (!basis || !coef)) || !G || !ell_joint || !ell_weight || !gV || !workspace) return CAPE_EINVAL;
    if (ell_width < 1 || ell_width > J) return CAPE_EINVAL;
    if (3LL * K * V >= (1LL << 31) || (int64_t)ell_width * V >= (1LL << 31)) return CAPE_EINVAL;   // 32-bit element index
    if (T_sample_stride < 0 || (T_sample_stride > 0 && T_sample_stride < 3LL * V) || gV_sample_stride < 3LL * V ||
        (q && q_sample_stride < 3LL * V))
        return CAPE_EINVAL;
    if (workspace_bytes < 4LL * N * plan[1] * plan[2]) return CAPE_EINVAL;
    const int32_t tile = plan[0], tiles = (N + tile - 1) / tile, threads = bwd_threads(tiles, V);
    dim3 grid(plan[1], tiles);
    const size_t lds = 4 * (size_t)(((K * tile + 3) & ~3) + 12 * J * tile + SMPL_BWD_XCH);
    if (need_coef && K > 0)
        smpl_skin_bwd_kernel<true><<<grid, threads, lds, (hipStream_t)stream>>>(T, T_sample_stride, basis, K, coef, G, ell_joint,
            ell_weight, ell_width, gV, gV_sample_stride, J, V, N, tile, q, q_sample_stride, (float *)workspace);
    else
        smpl_skin_bwd_kernel<false><<<grid, threads, lds, (hipStream_t)stream>>>(T, T_sample_stride, basis, K, coef, G, ell_joint,
            ell_weight, ell_width, gV, gV_sample_stride, J, V, N, tile, q, q_sample_stride, (float *)workspace);
    return launch_status();
}

extern "C" int cape_smpl_joints_bwd(const float *T, int64_t T_sample_stride, const int32_t *jreg_rowptr,
                                    const int32_t *jreg_colidx, const float *jreg_vals, const float *pose, const float *betas,
                                    int32_t B, const float *jshapedirs, const int32_t *parents, int32_t J, int32_t V, int32_t N,
                                    const float *gJ, const void *partials, int32_t blocks, int32_t coef_valid, float *dpose,
                                    float *dbetas, float *dtransl, float *dJn, void *stream) {
    SmplTree tree;
    const int rc = smpl_tree(parents, J, &tree);
    if (rc) return rc;
    if (!T || !jreg_rowptr || !jreg_colidx || !jreg_vals || !pose) return CAPE_EINVAL;
    if (B < 0 || (B > 0 && (!betas || !jshapedirs))) return CAPE_EINVAL;
    if (N < 1 || V < 1 || V > (1 << 29) || T_sample_stride < 0 || (T_sample_stride > 0 && T_sample_stride < 3LL * V))
        return CAPE_EINVAL;
    if ((!gJ && !partials) || (partials && blocks < 1) || (!dpose && !dbetas && !dtransl && !dJn)) return CAPE_EINVAL;
    // without the vertex pass's gcoef sums the partials' first K words are unwritten: pose and shape gradients need them
    if (partials && !coef_valid && (dpose || (dbetas && B > 0))) return CAPE_EINVAL;
    smpl_joints_bwd_kernel<<<N, 256, 0, (hipStream_t)stream>>>(T, T_sample_stride, jreg_rowptr, jreg_colidx, jreg_vals, pose, betas,
                                                               B, jshapedirs, tree, gJ, (const float *)partials, blocks, coef_valid, dpose,
                                                               B > 0 ? dbetas : nullptr, dtransl, dJn);
    return launch_status();
}

extern "C" int cape_smpl_jreg_bwd(const float *q, int64_t q_sample_stride, const int32_t *jregT_colptr,
                                  const int32_t *jregT_rowidx, const float *jregT_vals, const float *dJn, int32_t J, int32_t V,
                                  int32_t N, int32_t shared, float *dT, int64_t dT_sample_stride, void *stream) {
    if (!jregT_colptr || !jregT_rowidx || !jregT_vals || !dJn || !dT) return CAPE_EINVAL;
    if (J < 1 || J > SMPL_MAX_J || N < 1 || N > 65535 || V < 1 || V > (1 << 29)) return CAPE_EINVAL;
    if ((q && q_sample_stride < 3LL * V) || (!shared && dT_sample_stride < 3LL * V)) return CAPE_EINVAL;
    dim3 grid((3 * V + 255) / 256, shared ? 1 : N);
    smpl_jreg_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(q, q_sample_stride, jregT_colptr, jregT_rowidx, jregT_vals, dJn, J,
                                                                3 * V, N, shared ? 1 : 0, dT, dT_sample_stride);
    return launch_status();
}

extern "C" int cape_smpl_dress_bwd(const float *g, int64_t g_sample_stride, const float *std_, const float *mask, float *d_disp,
                                   int64_t d_sample_stride, int32_t N, int32_t V, void *stream) {
    if (!g || !std_ || !mask || !d_disp) return CAPE_EINVAL;
    if (N < 1 || N > 65535 || V < 1 || V > (1 << 29)) return CAPE_EINVAL;
    if (g_sample_stride < 3LL * V || d_sample_stride < 3LL * V) return CAPE_EINVAL;
    dim3 grid((3 * V + 255) / 256, N);
    smpl_dress_bwd_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(g, g_sample_stride, std_, mask, d_disp, d_sample_stride, 3 * V);
    return launch_status();
}

extern "C" int cape_smpl_weighted_l2(const float *pred, int64_t pred_sample_stride, const float *target,
                                     int64_t target_sample_stride, const float *weights, float inv_weight_sum, int32_t N,
                                     int32_t V, float *loss, float *grad, int64_t grad_sample_stride, void *stream) {
    if (!pred || !target || !weights || !loss) return CAPE_EINVAL;
    if (N < 1 || V < 1 || V > (1 << 29)) return CAPE_EINVAL;
    if (pred_sample_stride < 3LL * V || target_sample_stride < 3LL * V || (grad && grad_sample_stride < 3LL * V)) return CAPE_EINVAL;
    smpl_weighted_l2_kernel<<<N, 256, 0, (hipStream_t)stream>>>(pred, pred_sample_stride, target, target_sample_stride, weights,
                                                                inv_weight_sum, V, loss, grad, grad_sample_stride);
    return launch_status();
}
