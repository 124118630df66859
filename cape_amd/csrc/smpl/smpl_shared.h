// What the SMPL posing forward (smpl.hip) and its backward (smpl_bwd.hip) share: the kinematic tree passed by value, Rodrigues'
// formula, and the joint regression + kinematic chain of one sample, which the backward recomputes exactly as the forward ran it.
#pragma once
#include "../common.h"

#define SMPL_MAX_J 64
#define SMPL_TILE 16            // samples per skinning workgroup (at most; fewer when their LDS does not fit)
#define SMPL_SKIN_LDS (64 * 1024)

// the kinematic tree, by value in the launch (a graph capture keeps it): parents[j] < j for j >= 1, depth[0] = 0
struct SmplTree {
    int32_t J, maxdepth;
    int8_t parent[SMPL_MAX_J];
    uint8_t depth[SMPL_MAX_J];
};

// |r|^2 as Rodrigues' formula takes it, and its test for the series branch: one definition, so that the backward takes the
// branch the forward took
__device__ __forceinline__ float smpl_theta2(float rx, float ry, float rz) { return rx * rx + ry * ry + rz * rz; }
__device__ __forceinline__ bool smpl_small_angle(float t2) { return t2 < 1e-6f; }

__device__ __forceinline__ void rodrigues(float rx, float ry, float rz, float *R) {
    // R = I + s K + c K^2, K = [r]_x, s = sin(t)/t, c = (1 - cos t)/t^2 = 2 (sin(t/2)/t)^2 (no cancellation at small t);
    // below t^2 = 1e-6 the series s = 1 - t^2/6, c = 1/2 - t^2/24 (truncation < 1e-13): exactly I at r = 0
    const float t2 = smpl_theta2(rx, ry, rz);
    float s, c;
    if (smpl_small_angle(t2)) {
        s = 1.f - t2 * (1.f / 6.f);
        c = 0.5f - t2 * (1.f / 24.f);
    } else {
        const float t = sqrtf(t2);
        s = sinf(t) / t;
        const float h = sinf(0.5f * t) / t;
        c = 2.f * h * h;
    }
    // K^2 = r r^T - t^2 I
    R[0] = 1.f + c * (rx * rx - t2); R[1] = -s * rz + c * (rx * ry);     R[2] = s * ry + c * (rx * rz);
    R[3] = s * rz + c * (ry * rx);     R[4] = 1.f + c * (ry * ry - t2); R[5] = -s * rx + c * (ry * rz);
    R[6] = -s * ry + c * (rz * rx);    R[7] = s * rx + c * (rz * ry);     R[8] = 1.f + c * (rz * rz - t2);
}

// Joints of sample n's rest body, the joint rotations and the chain, by a workgroup of 256 threads; ends on a barrier:
//   sJ = J_regressor . T + jsd . betas,  sR[j] = Rodrigues(pose_j),  sA[j] = [rot 3x3 row-major | t]: A_0 = [R_0 | J_0],
//   A_j = A_p [R_j | J_j - J_p]
__device__ __forceinline__ void smpl_chain(const float *__restrict__ Tn, const int32_t *__restrict__ rp,
                                           const int32_t *__restrict__ ci, const float *__restrict__ cv,
                                           const float *__restrict__ pn, const float *__restrict__ bn, int32_t B,
                                           const float *__restrict__ jsd, const SmplTree &tree, float (*sJ)[3], float (*sR)[9],
                                           float (*sA)[12]) {
    const int32_t J = tree.J, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // J_regressor . T: one wave per joint, lanes over the row in a fixed order, a fixed butterfly across the wave
    for (int32_t j = wave; j < J; j += 4) {
        float ax = 0.f, ay = 0.f, az = 0.f;
        for (int32_t e = rp[j] + lane; e < rp[j + 1]; e += 64) {
            const float w = cv[e];
            const float *p = Tn + 3 * (int64_t)ci[e];
            ax += w * p[0]; ay += w * p[1]; az += w * p[2];
        }
#pragma unroll
        for (int32_t o = 32; o > 0; o >>= 1) {
            ax += __shfl_xor(ax, o); ay += __shfl_xor(ay, o); az += __shfl_xor(az, o);
        }
        if (lane == 0) { sJ[j][0] = ax; sJ[j][1] = ay; sJ[j][2] = az; }
    }
    __syncthreads();
    // + (J_regressor . shapedirs) . betas, jsd [B][J][3]
    if (tid < 3 * J) {
        float a = sJ[tid / 3][tid % 3];
        for (int32_t b = 0; b < B; ++b) a += bn[b] * jsd[b * 3 * J + tid];
        sJ[tid / 3][tid % 3] = a;
    }
    if (tid < J) {
        float R[9];
        rodrigues(pn[3 * tid], pn[3 * tid + 1], pn[3 * tid + 2], R);
#pragma unroll
        for (int32_t q = 0; q < 9; ++q) sR[tid][q] = R[q];
    }
    __syncthreads();
    // the chain, level by level
    if (tid == 0) {
#pragma unroll
        for (int32_t r = 0; r < 3; ++r) {
            sA[0][4 * r] = sR[0][3 * r]; sA[0][4 * r + 1] = sR[0][3 * r + 1]; sA[0][4 * r + 2] = sR[0][3 * r + 2];
            sA[0][4 * r + 3] = sJ[0][r];
        }
    }
    __syncthreads();
    for (int32_t lvl = 1; lvl <= tree.maxdepth; ++lvl) {
        if (tid < J && tree.depth[tid] == lvl) {
            const int32_t p = tree.parent[tid];
            const float d0 = sJ[tid][0] - sJ[p][0], d1 = sJ[tid][1] - sJ[p][1], d2 = sJ[tid][2] - sJ[p][2];
#pragma unroll
            for (int32_t r = 0; r < 3; ++r) {
                const float a0 = sA[p][4 * r], a1 = sA[p][4 * r + 1], a2 = sA[p][4 * r + 2];
#pragma unroll
                for (int32_t c = 0; c < 3; ++c) sA[tid][4 * r + c] = a0 * sR[tid][c] + a1 * sR[tid][3 + c] + a2 * sR[tid][6 + c];
                sA[tid][4 * r + 3] = a0 * d0 + a1 * d1 + a2 * d2 + sA[p][4 * r + 3];
            }
        }
        __syncthreads();
    }
}

static int smpl_tree(const int32_t *parents, int32_t J, SmplTree *t) {
    if (!parents || J < 1 || J > SMPL_MAX_J) return CAPE_EINVAL;
    if (parents[0] != -1) return CAPE_ERANGE;
    t->J = J;
    t->maxdepth = 0;
    t->parent[0] = -1;
    t->depth[0] = 0;
    for (int32_t j = 1; j < J; ++j) {
        if (parents[j] < 0 || parents[j] >= j) return CAPE_ERANGE;
        t->parent[j] = (int8_t)parents[j];
        t->depth[j] = (uint8_t)(t->depth[parents[j]] + 1);
        if (t->depth[j] > t->maxdepth) t->maxdepth = t->depth[j];
    }
    return CAPE_OK;
}

static int launch_status() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? CAPE_OK : (int)e;
}
