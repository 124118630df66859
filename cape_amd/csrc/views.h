// What elementwise.hip and sparse.hip share: the [N, M, ld] view of a tensor, the alignment tests that pick a vector form, and
// the row-bound conventions of the kernels that own whole rows.
#pragma once
#include "common.h"

namespace {

template <typename T> struct ViewT {
    T *p;
    long long ss;
    int ld;
};
template <typename T> struct CViewT {
    const T *p;
    long long ss;
    int ld;
};
typedef ViewT<float> View;
typedef CViewT<float> CView;

// four consecutive elements addressable as one vector access (16 bytes of fp32, 8 bytes of bf16)
__host__ __device__ inline bool aligned4(const void *p, long long ss, int ld, int C, int es = 4) {
    return ((reinterpret_cast<uintptr_t>(p) & (4 * es - 1)) == 0) && ((ss & 3) == 0) && ((ld & 3) == 0) && ((C & 3) == 0);
}
// eight consecutive elements addressable as vector accesses (fp32: two 16-byte accesses, bf16: one)
inline bool aligned8(const void *p, long long ss, int ld, int C, int es) {
    const int a = es == 4 ? 3 : 7;          // element alignment of the row starts
    return ((reinterpret_cast<uintptr_t>(p) & 15) == 0) && ((ss & a) == 0) && ((ld & a) == 0) && ((C & 7) == 0);
}

#ifndef CAPE_SPMM_WIDE_DEFAULT
#define CAPE_SPMM_WIDE_DEFAULT 1
#endif
// CAPE_SPMM_WIDE (A/B switch, read once) = 1: 8 channels per work item where the channel count and the alignment allow, 0: always 4
inline bool spmm_wide() {
    static const int w = getenv("CAPE_SPMM_WIDE") ? atoi(getenv("CAPE_SPMM_WIDE")) : CAPE_SPMM_WIDE_DEFAULT;
    return w != 0;
}

// Row bounds of an output (cape_h2_src_t.rowmax, width 4): written by the kernel itself when the lanes of a row form one aligned
// power-of-two group inside a wave, otherwise by one standalone pass over the finished output (csrc/pieces.hip).
inline bool rm_fused(int lanes_per_row) { return lanes_per_row >= 1 && lanes_per_row <= 64 && (lanes_per_row & (lanes_per_row - 1)) == 0; }
template <typename T>
inline int rm_standalone(const T *y, int64_t ys, int32_t ldy, int32_t N, int32_t Mo, int32_t C, float *rowmax_out, void *stream) {
    if (sizeof(T) != 4) return CAPE_EINVAL;
    return cape_rowmax(reinterpret_cast<const float *>(y), ys, ldy, N, Mo, C, rowmax_out, 4, stream);
}

}  // namespace
