// azr_train_gemm.hpp — the optimiser step's GEMM on the fp32 MFMA (t_gemm) and its tile loaders
// (A private header of azr_train.hip, the one translation unit that includes it: everything here has internal linkage.)
#pragma once
#include <hip/hip_runtime.h>
#include "azr_train_common.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// =====================================================================================================================
// GEMM  C[M][N] = A[M][K] x B[K][N]  on v_mfma_f32_32x32x2_f32.  128x128 block tile, 4 waves of 64x64 (2x2 MFMA tiles),
// k-tile 16 staged in LDS as [k][m|n] so an MFMA operand read is 32 consecutive floats.  Operand storage is a template
// switch: A_MCONTIG = A stored [K][M] (column access of a row-major matrix, used for col^T), B_KCONTIG = B stored [N][K]
// (W^T).  blockIdx.z = split-K slice writing C + z * strideCz.  All edges are bounds-checked.
// =====================================================================================================================
constexpr int GT = 128, GK = 16, GLD = GT + 4;

// tile loaders: a [GK][T] tile (T = 128 or 64 along m|n), T * GK / 256 floats per thread.  MODE selects the operand view:
//   0  plain matrix: element (mn, k) at P[k * ld + mn] (MN_CONTIG) or P[mn * ld + k]
//   1  implicit im2col of an activation P [rows][256]: the matrix col[row][tap * 256 + c] = P[row + off(tap)][c] inside
//      the board, 0 outside (never materialised); "row" is mn when !MN_CONTIG (forward A) and k when MN_CONTIG (col^T)
//   2  the same with the tap offsets negated (the transposed convolution of the backward-data pass)
//   3  conv kernel W [tap][ci][co] viewed as B[k = tap * 256 + co][n = ci] (backward-data), !MN_CONTIG only
template <bool MN_CONTIG, int T, int MODE>
__device__ __forceinline__ void gt_load(const float* __restrict__ P, int ld, int mn0, int k0, int MN, int Kend, int t, float (&r)[T / 16])
{
    constexpr int V = T / 16;  // 8 or 4 floats per thread
    constexpr int TPR = 16 / V;
    const int mn = MN_CONTIG ? mn0 + (t & 15) * V : mn0 + t / TPR;
    const int k = MN_CONTIG ? k0 + (t >> 4) : k0 + (t % TPR) * V;
    const float* p;
    bool ok;  // the whole run of V elements is inside the matrix (runs never straddle: all extents are multiples of V)
    if constexpr (MODE == 1 || MODE == 2) {
        const int row = MN_CONTIG ? k : mn, kk = MN_CONTIG ? mn : k;  // kk = tap * 256 + c
        const int tap = kk >> 8, c = kk & 255;
        int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
        if (MODE == 2) { dy = -dy; dx = -dx; }
        const int pos = row % NPOS, y = pos / 6 + dy, x = pos - (pos / 6) * 6 + dx;
        ok = (MN_CONTIG ? (row < Kend && kk < MN) : (row < MN && kk < Kend)) && y >= 0 && y < 7 && x >= 0 && x < 6;
        p = P + (size_t)(row + dy * 6 + dx) * NF + c;
#pragma unroll
        for (int j = 0; j < V; j++) r[j] = 0.0f;
        if (ok) {
#pragma unroll
            for (int q = 0; q < V / 4; q++) {
                const float4 a = reinterpret_cast<const float4*>(p)[q];
                r[4 * q] = a.x; r[4 * q + 1] = a.y; r[4 * q + 2] = a.z; r[4 * q + 3] = a.w;
            }
        }
        return;
    } else if constexpr (MODE == 3) {
        static_assert(!MN_CONTIG, "weight-tap view is k-contiguous");
        p = P + (size_t)(k >> 8) * (NF * NF) + (size_t)mn * NF + (k & 255);
        ok = mn < MN && k + V - 1 < Kend;
    } else if constexpr (MN_CONTIG) {
        p = P + (size_t)k * ld + mn;
        ok = k < Kend && mn + V - 1 < MN;
    } else {
        p = P + (size_t)mn * ld + k;
        ok = mn < MN && k + V - 1 < Kend;
    }
    if (ok) {
#pragma unroll
        for (int q = 0; q < V / 4; q++) {
            const float4 a = reinterpret_cast<const float4*>(p)[q];
            r[4 * q] = a.x; r[4 * q + 1] = a.y; r[4 * q + 2] = a.z; r[4 * q + 3] = a.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; j++) {
            const bool in = MN_CONTIG ? (k < Kend && mn + j < MN) : (mn < MN && k + j < Kend);
            r[j] = (MODE == 0 && in) ? p[j] : 0.0f;
        }
    }
}

template <bool MN_CONTIG, int T>
__device__ __forceinline__ void gt_store(float* S, int t, const float (&r)[T / 16])
{
    constexpr int V = T / 16, LD = T + 4;
    if constexpr (MN_CONTIG) {
        float* p = S + (t >> 4) * LD + (t & 15) * V;
#pragma unroll
        for (int q = 0; q < V / 4; q++) reinterpret_cast<float4*>(p)[q] = make_float4(r[4 * q], r[4 * q + 1], r[4 * q + 2], r[4 * q + 3]);
    } else {
        constexpr int TPR = 16 / V;
        float* p = S + ((t % TPR) * V) * LD + t / TPR;
#pragma unroll
        for (int j = 0; j < V; j++) p[j * LD] = r[j];
    }
}

// BM = 128: 4 waves as 2 x 2, each 64 x 64 (2 x 2 MFMA tiles); BM = 64: 2 x 2 waves, each 32 x 64 (1 x 2 tiles) — the
// smaller tile is for launches whose 128-row grid would leave CUs with 1 vs 2 blocks (forward conv: 336 -> 672 blocks)
template <bool A_MCONTIG, bool B_KCONTIG, int BM, int AMODE, int BMODE>
__global__ __launch_bounds__(256) void t_gemm(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                                              float* __restrict__ C, int ldc, int M, int N, int K, int kchunk, size_t strideCz)
{
    constexpr int MI = BM / 64, LDA = BM + 4;
    __shared__ __attribute__((aligned(16))) float As[GK * LDA];
    __shared__ __attribute__((aligned(16))) float Bs[GK * GLD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * GT;
    const int kbeg = blockIdx.z * kchunk, kend = min(K, kbeg + kchunk);
    f32x16 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[i][j][e] = 0.0f;
    float ra[BM / 16], rb[8];
    gt_load<A_MCONTIG, BM, AMODE>(A, lda, m0, kbeg, M, kend, t, ra);
    gt_load<!B_KCONTIG, GT, BMODE>(B, ldb, n0, kbeg, N, kend, t, rb);
    for (int k0 = kbeg; k0 < kend; k0 += GK) {
        __syncthreads();
        gt_store<A_MCONTIG, BM>(As, t, ra);
        gt_store<!B_KCONTIG, GT>(Bs, t, rb);
        __syncthreads();
        if (k0 + GK < kend) {
            gt_load<A_MCONTIG, BM, AMODE>(A, lda, m0, k0 + GK, M, kend, t, ra);
            gt_load<!B_KCONTIG, GT, BMODE>(B, ldb, n0, k0 + GK, N, kend, t, rb);
        }
#pragma unroll
        for (int kk = 0; kk < GK / 2; kk++) {
            const int k = kk * 2 + (lane >> 5);
            float a[MI];
#pragma unroll
            for (int i = 0; i < MI; i++) a[i] = As[k * LDA + wm * (32 * MI) + i * 32 + (lane & 31)];
            const float b0 = Bs[k * GLD + wn * 64 + (lane & 31)], b1 = Bs[k * GLD + wn * 64 + 32 + (lane & 31)];
#pragma unroll
            for (int i = 0; i < MI; i++) {
                acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b0, acc[i][0], 0, 0, 0);
                acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b1, acc[i][1], 0, 0, 0);
            }
        }
    }
    float* Cz = C + (size_t)blockIdx.z * strideCz;
#pragma unroll
    for (int i = 0; i < MI; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int row = m0 + wm * (32 * MI) + i * 32 + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
                const int col = n0 + wn * 64 + j * 32 + (lane & 31);
                if (row < M && col < N) Cz[(size_t)row * ldc + col] = acc[i][j][e];
            }
}

}  // namespace
