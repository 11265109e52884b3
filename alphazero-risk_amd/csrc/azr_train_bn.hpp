// azr_train_bn.hpp — batch normalisation (training mode, forward and backward; moving statistics for the validation pass) and the heads
// (A private header of azr_train.hip, the one translation unit that includes it: everything here has internal linkage.)
#pragma once
#include "azr_train_conv.hpp"

namespace {

// =====================================================================================================================
// batch normalisation, training mode.  STEM = the conv_bn layer normalising over axis 1 = board row y (7 groups,
// build_graph.py:68); otherwise per channel.  Stage 1: per block of RB rows, thread c accumulates in double; stage 2: one
// block sums the partials.
// =====================================================================================================================
constexpr int NG = 7;  // stem groups

// sum of v over the 4 row-groups q = t >> 8 of a 1024-thread block, per channel c = t & 255 (result valid where q == 0)
__device__ __forceinline__ double reduce_q4(double v, double* sh)
{
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    if (t < 256) v = sh[t] + sh[t + 256] + sh[t + 512] + sh[t + 768];
    return v;
}

// sum of v over the 32 row-groups q = t >> 5 of a 1024-thread block, per channel slot t & 31 (valid where q == 0)
__device__ __forceinline__ double reduce_q32(double v, double* sh)
{
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int o = 512; o >= 32; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    return sh[t & 31];
}

__device__ __forceinline__ double block_sum_1024(double v, double* sh)
{
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (t < o) sh[t] += sh[t + o];
        __syncthreads();
    }
    return sh[0];
}

template <bool STEM>
__global__ __launch_bounds__(1024) void t_bn_stats(const float* __restrict__ Y, int M, double* __restrict__ part)
{
    __shared__ double sh[1024];
    const int c = threadIdx.x & 255, q = threadIdx.x >> 8, r0 = blockIdx.x * RB, r1 = min(M, r0 + RB);
    if constexpr (!STEM) {
        double s = 0.0, ss = 0.0;
#pragma unroll 4
        for (int r = r0 + q; r < r1; r += 4) bn_stat_fwd(Y[(size_t)r * NF + c], s, ss);
        s = reduce_q4(s, sh);
        ss = reduce_q4(ss, sh);
        if (q == 0) {
            part[((size_t)blockIdx.x * 2 + 0) * NF + c] = s;
            part[((size_t)blockIdx.x * 2 + 1) * NF + c] = ss;
        }
    } else {
        double s[NG], ss[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) s[g] = ss[g] = 0.0;
        for (int r = r0 + q; r < r1; r += 4) {
            const double v = Y[(size_t)r * NF + c];
            const int y = (r % NPOS) / 6;
#pragma unroll
            for (int g = 0; g < NG; g++) { s[g] += y == g ? v : 0.0; ss[g] += y == g ? v * v : 0.0; }
        }
#pragma unroll
        for (int g = 0; g < NG; g++) {
            const double a = reduce_q4(s[g], sh), b = reduce_q4(ss[g], sh);
            if (q == 0) {
                part[((size_t)blockIdx.x * 2 * NG + g) * NF + c] = a;
                part[((size_t)blockIdx.x * 2 * NG + NG + g) * NF + c] = b;
            }
        }
    }
}

// mean / 1/sqrt(var+eps) of the batch + moving-average update (TF fused BN: moving variance gets Bessel's correction)
template <bool STEM>
__global__ __launch_bounds__(1024) void t_bn_finalize(const double* __restrict__ part, int R, double count, float* __restrict__ mean,
                                                      float* __restrict__ istd, float* __restrict__ bn /* g|b|mu|var */)
{
    __shared__ double sh[1024];
    int c = threadIdx.x & 255, q = threadIdx.x >> 8;
    if constexpr (!STEM) {
        // grid of 8 blocks: block = 32 channels x 32 groups of partial rows
        c = blockIdx.x * 32 + (threadIdx.x & 31);
        q = threadIdx.x >> 5;
        double s = 0.0, ss = 0.0;
        for (int b = q; b < R; b += 32) { s += part[((size_t)b * 2 + 0) * NF + c]; ss += part[((size_t)b * 2 + 1) * NF + c]; }
        s = reduce_q32(s, sh);
        ss = reduce_q32(ss, sh);
        if (q == 0) {
            const double mu = s / count, var = fmax(ss / count - mu * mu, 0.0);
            mean[c] = (float)mu;
            istd[c] = (float)(1.0 / sqrt(var + (double)BN_EPS));
            bn[2 * NF + c] = bn[2 * NF + c] * BN_KEEP + (float)mu * (1.0f - BN_KEEP);
            bn[3 * NF + c] = bn[3 * NF + c] * BN_KEEP + (float)(var * count / (count - 1.0)) * (1.0f - BN_KEEP);
        }
    } else {
        {   // grid of NG blocks: one board row each (the sums of a row keep their order)
            const int g = blockIdx.x;
            double s = 0.0, ss = 0.0;
#pragma unroll 8
            for (int b = q; b < R; b += 4) {
                s += part[((size_t)b * 2 * NG + g) * NF + c];
                ss += part[((size_t)b * 2 * NG + NG + g) * NF + c];
            }
            s = block_sum_1024(s, sh);
            ss = block_sum_1024(ss, sh);
            if (threadIdx.x == 0) {
                const double mu = s / count, var = fmax(ss / count - mu * mu, 0.0);
                mean[g] = (float)mu;
                istd[g] = (float)(1.0 / sqrt(var + (double)BN_EPS));
                bn[2 * NG + g] = bn[2 * NG + g] * BN_KEEP + (float)mu * (1.0f - BN_KEEP);
                bn[3 * NG + g] = bn[3 * NG + g] * BN_KEEP + (float)(var * count / (count - 1.0)) * (1.0f - BN_KEEP);
            }
        }
    }
}

// A = relu(gamma * (Y - mean) * istd + beta (+ S))
template <bool STEM>
__global__ __launch_bounds__(256) void t_bn_apply(const float* __restrict__ Y, const float* __restrict__ mean, const float* __restrict__ istd,
                                                  const float* __restrict__ bn, const float* __restrict__ S, float* __restrict__ A, int M,
                                                  uint16_t* __restrict__ p0, uint16_t* __restrict__ p1, uint16_t* __restrict__ p2,
                                                  uint16_t* __restrict__ q0 = nullptr, uint16_t* __restrict__ q1 = nullptr)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // float4 index
    if (i >= (size_t)M * (NF / 4)) return;
    const int r = (int)(i / (NF / 4)), c4 = (int)(i % (NF / 4)) * 4;
    const int CH = STEM ? NG : NF;
    const float4 y = reinterpret_cast<const float4*>(Y)[i];
    const float4 s = S ? reinterpret_cast<const float4*>(S)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float yy[4] = {y.x, y.y, y.z, y.w}, sv[4] = {s.x, s.y, s.z, s.w};
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int ch = STEM ? (r % NPOS) / 6 : c4 + j;
        o[j] = bn_fwd(yy[j], sv[j], bn[ch], bn[CH + ch], mean[ch], istd[ch]);
    }
    reinterpret_cast<float4*>(A)[i] = make_float4(o[0], o[1], o[2], o[3]);
    if (p0) split_store4(o, i, p0, p1, p2);  // bf16 parts: the weight-gradient GEMM's operand (and, with p2, the 6-pass forward conv's)
    if (q0) split_store4_f16(o, i, q0, q1);  // fp16 pair: the next layer's 3-pass forward conv
}

// inference mode (the validation pass, azr_nn_validate): mean / 1/sqrt(var+eps) of every BN layer taken from its MOVING statistics in
// the AZRW vector w (read only), in the slots t_bn_finalize fills with batch statistics — block 0 the stem's 7 rows, block l of 1 .. L-1
// conv layer l, block L the three head channels (hstat) — so that the forward kernels run unchanged
__global__ __launch_bounds__(256) void t_bn_moving(const float* __restrict__ w, int L, float* __restrict__ mean, float* __restrict__ istd,
                                                   float* __restrict__ hstat)
{
    const int l = blockIdx.x, t = threadIdx.x;
    auto inv_std = [](float var) { return (float)(1.0 / sqrt((double)var + (double)BN_EPS)); };
    if (l == 0) {
        const float* bn = w + OFF_STEM_BN;   // g | b | mu | var, 7 each
        if (t < NG) { mean[t] = bn[2 * NG + t]; istd[t] = inv_std(bn[3 * NG + t]); }
    } else if (l < L) {
        const float* bn = w + OFF_BLOCK0 + (size_t)(l - 1) * LAYER + (size_t)9 * NF * NF;
        mean[l * NF + t] = bn[2 * NF + t];
        istd[l * NF + t] = inv_std(bn[3 * NF + t]);
    } else if (t < 3) {
        const float* hp = w + OFF_BLOCK0 + (size_t)(L - 1) * LAYER;
        const float* bn = t < 2 ? hp + H_PI_BN : hp + H_V_BN;
        const int C = t < 2 ? 2 : 1, k = t < 2 ? t : 0;
        hstat[t] = bn[2 * C + k];
        hstat[3 + t] = inv_std(bn[3 * C + k]);
    }
}

// backward stage 1: dz = dOut * (Apost > 0); partial sums of dz and dz * xhat
template <bool STEM>
__global__ __launch_bounds__(1024) void t_bn_bwd_stats(const float* __restrict__ dOut, const float* __restrict__ Apost,
                                                       const float* __restrict__ Y, const float* __restrict__ mean,
                                                       const float* __restrict__ istd, int M, double* __restrict__ part)
{
    __shared__ double sh[1024];
    const int c = threadIdx.x & 255, q = threadIdx.x >> 8, r0 = blockIdx.x * RB, r1 = min(M, r0 + RB);
    if constexpr (!STEM) {
        const float mu = mean[c], is = istd[c];
        double s = 0.0, sx = 0.0;
#pragma unroll 4
        for (int r = r0 + q; r < r1; r += 4) {
            const size_t i = (size_t)r * NF + c;
            bn_stat_bwd(Apost[i] > 0.0f ? dOut[i] : 0.0f, Y[i], mu, is, s, sx);
        }
        s = reduce_q4(s, sh);
        sx = reduce_q4(sx, sh);
        if (q == 0) {
            part[((size_t)blockIdx.x * 2 + 0) * NF + c] = s;
            part[((size_t)blockIdx.x * 2 + 1) * NF + c] = sx;
        }
    } else {
        double s[NG], sx[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) s[g] = sx[g] = 0.0;
        for (int r = r0 + q; r < r1; r += 4) {
            const size_t i = (size_t)r * NF + c;
            const int y = (r % NPOS) / 6;
            const float dz = Apost[i] > 0.0f ? dOut[i] : 0.0f;
            const double x = (double)dz * (double)bn_xhat(Y[i], mean[y], istd[y]);
#pragma unroll
            for (int g = 0; g < NG; g++) { s[g] += y == g ? (double)dz : 0.0; sx[g] += y == g ? x : 0.0; }
        }
#pragma unroll
        for (int g = 0; g < NG; g++) {
            const double a = reduce_q4(s[g], sh), b = reduce_q4(sx[g], sh);
            if (q == 0) {
                part[((size_t)blockIdx.x * 2 * NG + g) * NF + c] = a;
                part[((size_t)blockIdx.x * 2 * NG + NG + g) * NF + c] = b;
            }
        }
    }
}

// data-parallel step: this rank's per-block partials -> one [K][256] slab of doubles, which the ranks then all-reduce; the
// finalize kernels read the reduced slab as "R = 1 block of partials"
__global__ __launch_bounds__(256) void t_parts_sum(const double* __restrict__ part, int R, int K, double* __restrict__ red)
{
    const int c = threadIdx.x, k = blockIdx.x;
    double s = 0.0;
    for (int b = 0; b < R; b++) s += part[((size_t)b * K + k) * NF + c];
    red[(size_t)k * NF + c] = s;
}

// backward stage 2: d(beta) = sum dz, d(gamma) = sum dz * xhat -> gradient vector; sums[0|1][ch] kept for stage 3.
// gscale = 1 / world in a data-parallel step (the sums are already global; the closing all-reduce of the gradient vector
// adds the `world` copies up again)
__device__ __forceinline__ void bn_bwd_finalize_block(const double* __restrict__ part, int R, float* __restrict__ gbn, float* __restrict__ sums,
                                                      float gscale, double* sh)
{   // one of 8 blocks: 32 channels x 32 groups of partial rows
    const int c = blockIdx.x * 32 + (threadIdx.x & 31), q = threadIdx.x >> 5;
    double s = 0.0, sx = 0.0;
    for (int b = q; b < R; b += 32) { s += part[((size_t)b * 2 + 0) * NF + c]; sx += part[((size_t)b * 2 + 1) * NF + c]; }
    s = reduce_q32(s, sh);
    sx = reduce_q32(sx, sh);
    if (q == 0) {
        gbn[c] = (float)sx * gscale;
        gbn[NF + c] = (float)s * gscale;
        sums[c] = (float)s;
        sums[NF + c] = (float)sx;
    }
}
template <bool STEM>
__global__ __launch_bounds__(1024) void t_bn_bwd_finalize(const double* __restrict__ part, int R, float* __restrict__ gbn, float* __restrict__ sums,
                                                          float gscale)
{
    __shared__ double sh[1024];
    if constexpr (!STEM) {
        bn_bwd_finalize_block(part, R, gbn, sums, gscale, sh);
    } else {   // grid of NG blocks: one board row each
        const int c = threadIdx.x & 255, q = threadIdx.x >> 8, g = blockIdx.x;
        double s = 0.0, sx = 0.0;
#pragma unroll 8
        for (int b = q; b < R; b += 4) {
            s += part[((size_t)b * 2 * NG + g) * NF + c];
            sx += part[((size_t)b * 2 * NG + NG + g) * NF + c];
        }
        s = block_sum_1024(s, sh);
        sx = block_sum_1024(sx, sh);
        if (threadIdx.x == 0) { gbn[g] = (float)sx * gscale; gbn[NG + g] = (float)s * gscale; sums[g] = (float)s; sums[NF + g] = (float)sx; }
    }
}

// Two small kernels of the backward chain in ONE launch: the slice sum of layer l + 1's weight gradient (out[i] = sum_z part[z][i],
// the job of t_sum_slices) and stage 2 of layer l's batch-norm backward (t_bn_bwd_finalize<false>, blocks 0 - 7).  They are neighbours in
// the stream and independent of each other — the finalize reads the block partials the backward-data conv of layer l + 1 left, the
// slice sum what that layer's weight-gradient kernel left — so one launch saves a kernel boundary (~3 us on the device) and hides the
// 5-us finalize under the 10-us sum: ~8 us per layer.
__global__ __launch_bounds__(1024) void t_sum_slices_fin(const float* __restrict__ wpart, int nz, size_t n, float* __restrict__ out,
                                                         const double* __restrict__ part, int R, float* __restrict__ gbn, float* __restrict__ sums,
                                                         float gscale)
{
    if (blockIdx.x < 8) {
        __shared__ double sh[1024];
        bn_bwd_finalize_block(part, R, gbn, sums, gscale, sh);
        return;
    }
    const size_t i = (size_t)(blockIdx.x - 8) * 1024 + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    for (int z = 0; z < nz; z++) s += wpart[(size_t)z * n + i];
    out[i] = s;
}

// backward stage 3: dY = gamma * istd * (dz - sum(dz)/n - xhat * sum(dz xhat)/n); dZ (optional) = dz for the shortcut
template <bool STEM>
__global__ __launch_bounds__(256) void t_bn_bwd_apply(const float* __restrict__ dOut, const float* __restrict__ Apost,
                                                      const float* __restrict__ Y, const float* __restrict__ mean,
                                                      const float* __restrict__ istd, const float* __restrict__ bn,
                                                      const float* __restrict__ sums, float inv_count, float* __restrict__ dY,
                                                      float* __restrict__ dZ, int M, uint16_t* __restrict__ p0, uint16_t* __restrict__ p1)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)M * (NF / 4)) return;
    const int r = (int)(i / (NF / 4)), c4 = (int)(i % (NF / 4)) * 4;
    const float4 d4 = reinterpret_cast<const float4*>(dOut)[i], a4 = reinterpret_cast<const float4*>(Apost)[i],
                 y4 = reinterpret_cast<const float4*>(Y)[i];
    const float d[4] = {d4.x, d4.y, d4.z, d4.w}, a[4] = {a4.x, a4.y, a4.z, a4.w}, y[4] = {y4.x, y4.y, y4.z, y4.w};
    float o[4], z[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int ch = STEM ? (r % NPOS) / 6 : c4 + j;
        o[j] = bn_bwd(d[j], a[j], y[j], bn[ch], mean[ch], istd[ch], sums[ch] * inv_count, sums[NF + ch] * inv_count, z[j]);
    }
    if (dY) reinterpret_cast<float4*>(dY)[i] = make_float4(o[0], o[1], o[2], o[3]);
    if (dZ) reinterpret_cast<float4*>(dZ)[i] = make_float4(z[0], z[1], z[2], z[3]);
    if (p0) split_store4(o, i, p0, p1, nullptr);  // operand parts of the two gradient GEMMs
}

// =====================================================================================================================
// heads (build_graph.py:76-98)
// =====================================================================================================================
// 1x1 convs: pv0[r] = { H[r] . pi_w[:,0], H[r] . pi_w[:,1], H[r] . v_w, 0 }; one wave per row
__global__ __launch_bounds__(256) void t_head_conv(const float* __restrict__ H, const float* __restrict__ hp, float* __restrict__ pv0, int M)
{
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    const float4 h = reinterpret_cast<const float4*>(H)[(size_t)r * 64 + lane];
    const float hv[4] = {h.x, h.y, h.z, h.w};
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int c = lane * 4 + j;
        s0 += hv[j] * hp[H_PI_W + c * 2];
        s1 += hv[j] * hp[H_PI_W + c * 2 + 1];
        s2 += hv[j] * hp[H_V_W + c];
    }
    for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    if (lane == 0) reinterpret_cast<float4*>(pv0)[r] = make_float4(s0, s1, s2, 0.0f);
}

// batch statistics of the 3 head channels (bn_pi x2, bn_v) + moving averages; single block of 1024 threads.
// Two stages so that a data-parallel step can all-reduce the six sums in between: hsum = {s[3], ss[3]} (doubles).
__global__ __launch_bounds__(1024) void t_head_bn_sums(const float* __restrict__ pv0, int M, double* __restrict__ hsum)
{
    __shared__ double sh[1024];
    for (int ch = 0; ch < 3; ch++) {
        double s = 0.0, ss = 0.0;
        for (int r = threadIdx.x; r < M; r += 1024) { const double v = pv0[(size_t)r * 4 + ch]; s += v; ss += v * v; }
        s = block_sum_1024(s, sh);
        ss = block_sum_1024(ss, sh);
        if (threadIdx.x == 0) { hsum[ch] = s; hsum[3 + ch] = ss; }
    }
}
__global__ void t_head_bn_stats(const double* __restrict__ hsum, double n, float* __restrict__ hp, float* __restrict__ hstat /* mean[3] istd[3] */)
{
    const int ch = threadIdx.x;
    if (ch >= 3 || blockIdx.x != 0) return;
    const double mu = hsum[ch] / n, var = fmax(hsum[3 + ch] / n - mu * mu, 0.0);
    hstat[ch] = (float)mu;
    hstat[3 + ch] = (float)(1.0 / sqrt(var + (double)BN_EPS));
    float* bn = ch < 2 ? hp + H_PI_BN : hp + H_V_BN;
    const int C = ch < 2 ? 2 : 1, k = ch < 2 ? ch : 0;
    bn[2 * C + k] = bn[2 * C + k] * BN_KEEP + (float)mu * (1.0f - BN_KEEP);
    bn[3 * C + k] = bn[3 * C + k] * BN_KEEP + (float)(var * n / (n - 1.0)) * (1.0f - BN_KEEP);
}

__device__ __forceinline__ float head_bn_relu(const float* hp, const float* hstat, float x, int ch)
{
    const float* bn = ch < 2 ? hp + H_PI_BN : hp + H_V_BN;
    const int C = ch < 2 ? 2 : 1, k = ch < 2 ? ch : 0;
    const float v = bn[k] * ((x - hstat[ch]) * hstat[3 + ch]) + bn[C + k];
    return v > 0.0f ? v : 0.0f;
}

// dense parts + losses; one block of 256 threads per board.  Saves fpi[84], fv[42], h1[256], v, prob[43].
__global__ __launch_bounds__(256) void t_head_fwd(const float* __restrict__ pv0, const float* __restrict__ hp, const float* __restrict__ hstat,
                                                  const float* __restrict__ pit, const float* __restrict__ zt, float* __restrict__ fpi,
                                                  float* __restrict__ fv, float* __restrict__ h1, float* __restrict__ vout,
                                                  float* __restrict__ prob, float* __restrict__ lossb)
{
    __shared__ float s_pi[84], s_v[42], s_h[256], s_l[44];
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < 126) {
        const int cell = t / 3, ch = t % 3;
        const float f = head_bn_relu(hp, hstat, pv0[((size_t)b * NPOS + cell) * 4 + ch], ch);
        if (ch < 2) { s_pi[cell * 2 + ch] = f; fpi[b * 84 + cell * 2 + ch] = f; }
        else { s_v[cell] = f; fv[b * 42 + cell] = f; }
    }
    __syncthreads();
    {   // dense_1 42 -> 256 + ReLU
        float a = hp[H_V1_B + t];
        for (int k = 0; k < 42; k++) a += s_v[k] * hp[H_V1_W + k * 256 + t];
        a = a > 0.0f ? a : 0.0f;
        s_h[t] = a;
        h1[b * 256 + t] = a;
    }
    if (t < 43) {  // dense 84 -> 43
        float a = hp[H_PD_B + t];
        for (int k = 0; k < 84; k++) a += s_pi[k] * hp[H_PD_W + k * 43 + t];
        s_l[t] = a;
    }
    __syncthreads();
    if (t == 0) {
        float mx = s_l[0];
        for (int j = 1; j < 43; j++) mx = fmaxf(mx, s_l[j]);
        float se = 0.0f;
        for (int j = 0; j < 43; j++) se += expf(s_l[j] - mx);
        const float lse = mx + logf(se);
        float lp = 0.0f;
        for (int j = 0; j < 43; j++) {
            prob[b * 43 + j] = expf(s_l[j] - lse);
            lp -= pit[b * 43 + j] * (s_l[j] - lse);
        }
        float a = hp[H_V2_B];
        for (int j = 0; j < 256; j++) a += s_h[j] * hp[H_V2_W + j];
        const float v = tanhf(a), dv = zt[b] - v;
        vout[b] = v;
        lossb[b * 2] = lp;
        lossb[b * 2 + 1] = dv * dv;
    }
}

// batch means of the two losses (softmax_cross_entropy / mean_squared_error reduce over the batch) -> loss[0..1];
// acc[0..1] += them (the epoch sums of alphazero_nn.cpp:393-394, float like the reference)
// (a data-parallel step sums its own boards, divides by the GLOBAL batch, all-reduces loss[0..1], then accumulates)
__global__ void t_loss(const float* __restrict__ lossb, int BS, int BS_global, float* __restrict__ loss)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float lp = 0.0f, lv = 0.0f;
    for (int b = 0; b < BS; b++) { lp += lossb[b * 2]; lv += lossb[b * 2 + 1]; }
    loss[0] = lp / (float)BS_global; loss[1] = lv / (float)BS_global;
}
__global__ void t_loss_acc(const float* __restrict__ loss, float* __restrict__ acc)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) { acc[0] += loss[0]; acc[1] += loss[1]; }
}

// The heads of the validation pass, fused: one block of 256 threads per board does t_head_conv's 1x1 convs (one wave per cell, the
// same lane sums and butterfly), the head BN from hstat (t_bn_moving: the moving statistics), then t_head_fwd's dense layers and
// losses — lossb[b] = {cross-entropy from the logits, (z - v)^2}.  Nothing for a backward pass is written.
__global__ __launch_bounds__(256) void t_head_eval(const float* __restrict__ H, const float* __restrict__ hp, const float* __restrict__ hstat,
                                                   const float* __restrict__ pit, const float* __restrict__ zt, float* __restrict__ lossb)
{
    __shared__ float s_pi[84], s_v[42], s_h[256], s_l[44];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int cell = wave; cell < NPOS; cell += 4) {
        const float4 h = reinterpret_cast<const float4*>(H)[((size_t)b * NPOS + cell) * 64 + lane];
        const float hv[4] = {h.x, h.y, h.z, h.w};
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int c = lane * 4 + j;
            s0 += hv[j] * hp[H_PI_W + c * 2];
            s1 += hv[j] * hp[H_PI_W + c * 2 + 1];
            s2 += hv[j] * hp[H_V_W + c];
        }
        for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
        if (lane == 0) {
            s_pi[cell * 2] = head_bn_relu(hp, hstat, s0, 0);
            s_pi[cell * 2 + 1] = head_bn_relu(hp, hstat, s1, 1);
            s_v[cell] = head_bn_relu(hp, hstat, s2, 2);
        }
    }
    __syncthreads();
    {   // dense_1 42 -> 256 + ReLU
        float a = hp[H_V1_B + t];
        for (int k = 0; k < 42; k++) a += s_v[k] * hp[H_V1_W + k * 256 + t];
        s_h[t] = a > 0.0f ? a : 0.0f;
    }
    if (t < 43) {  // dense 84 -> 43
        float a = hp[H_PD_B + t];
        for (int k = 0; k < 84; k++) a += s_pi[k] * hp[H_PD_W + k * 43 + t];
        s_l[t] = a;
    }
    __syncthreads();
    if (t == 0) {
        float mx = s_l[0];
        for (int j = 1; j < 43; j++) mx = fmaxf(mx, s_l[j]);
        float se = 0.0f;
        for (int j = 0; j < 43; j++) se += expf(s_l[j] - mx);
        const float lse = mx + logf(se);
        float lp = 0.0f;
        for (int j = 0; j < 43; j++) lp -= pit[b * 43 + j] * (s_l[j] - lse);
        float a = hp[H_V2_B];
        for (int j = 0; j < 256; j++) a += s_h[j] * hp[H_V2_W + j];
        const float dv = zt[b] - tanhf(a);
        lossb[b * 2] = lp;
        lossb[b * 2 + 1] = dv * dv;
    }
}

// per-batch means of the validation pass, t_loss's arithmetic: batch k (one block) = lossb + k * 2 BS; the terms are staged in LDS
// by the block and summed in board order by one thread per loss -> means[k] = {sum(ce) / BS, sum(se) / BS}
constexpr int VM_CHUNK = 1024;   // boards per LDS stage
__global__ __launch_bounds__(256) void t_val_means(const float* __restrict__ lossb, int BS, float* __restrict__ means)
{
    __shared__ float s[2 * VM_CHUNK];
    const int k = blockIdx.x, t = threadIdx.x;
    const float* lb = lossb + (size_t)k * 2 * BS;
    float acc = 0.0f;
    for (int b0 = 0; b0 < BS; b0 += VM_CHUNK) {
        const int nb = min(VM_CHUNK, BS - b0);
        __syncthreads();
        for (int i = t; i < 2 * nb; i += 256) s[i] = lb[2 * b0 + i];
        __syncthreads();
        if (t < 2)
            for (int b = 0; b < nb; b++) acc += s[2 * b + t];
    }
    if (t < 2) means[(size_t)k * 2 + t] = acc / (float)BS;
}
// out[0..1] = the float sums of the batch means in batch order (t_loss_acc's accumulation)
__global__ void t_val_sum(const float* __restrict__ means, int nbatch, float* __restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float lp = 0.0f, lv = 0.0f;
    for (int k = 0; k < nbatch; k++) { lp += means[2 * k]; lv += means[2 * k + 1]; }
    out[0] = lp; out[1] = lv;
}

// backward of the dense parts; writes dz of the three head BN outputs (dpv [M][4]) and the per-board parameter partials
__global__ __launch_bounds__(256) void t_head_bwd(const float* __restrict__ hp, const float* __restrict__ pit, const float* __restrict__ zt,
                                                  const float* __restrict__ fpi, const float* __restrict__ fv, const float* __restrict__ h1,
                                                  const float* __restrict__ vout, const float* __restrict__ prob, int BS,
                                                  float* __restrict__ dpv, float* __restrict__ hpart)
{
    __shared__ float s_dl[43], s_dh[256], s_pi[84], s_v[42];
    __shared__ float s_dv;
    const int b = blockIdx.x, t = threadIdx.x;
    const float inv = 1.0f / (float)BS;
    float* hpb = hpart + (size_t)b * HP_FLOATS;
    if (t < 84) s_pi[t] = fpi[b * 84 + t];
    if (t < 42) s_v[t] = fv[b * 42 + t];
    if (t == 0) {
        float sp = 0.0f;
        for (int j = 0; j < 43; j++) sp += pit[b * 43 + j];
        for (int j = 0; j < 43; j++) s_dl[j] = (prob[b * 43 + j] * sp - pit[b * 43 + j]) * inv;
        const float v = vout[b];
        s_dv = 2.0f * (v - zt[b]) * inv * (1.0f - v * v);
    }
    __syncthreads();
    const float dv = s_dv;
    {
        const float h = h1[b * 256 + t];
        const float dh = h > 0.0f ? hp[H_V2_W + t] * dv : 0.0f;
        s_dh[t] = dh;
        hpb[HP_V1_B + t] = dh;
        hpb[HP_V2_W + t] = h * dv;
        if (t == 0) hpb[HP_V2_B] = dv;
        if (t < 43) hpb[HP_PD_B + t] = s_dl[t];
    }
    __syncthreads();
    for (int i = t; i < 84 * 43; i += 256) hpb[HP_PD_W + i] = s_pi[i / 43] * s_dl[i % 43];
    for (int i = t; i < 42 * 256; i += 256) hpb[HP_V1_W + i] = s_v[i / 256] * s_dh[i % 256];
    if (t < 84) {  // d fpi -> dz of bn_pi
        float a = 0.0f;
        for (int j = 0; j < 43; j++) a += hp[H_PD_W + t * 43 + j] * s_dl[j];
        dpv[((size_t)b * NPOS + t / 2) * 4 + (t & 1)] = s_pi[t] > 0.0f ? a : 0.0f;
    } else if (t >= 128 && t < 128 + 42) {  // d fv -> dz of bn_v
        const int k = t - 128;
        float a = 0.0f;
        for (int j = 0; j < 256; j++) a += hp[H_V1_W + k * 256 + j] * s_dh[j];
        dpv[((size_t)b * NPOS + k) * 4 + 2] = s_v[k] > 0.0f ? a : 0.0f;
    }
}

// g[param] = sum over boards of the per-board partials
__global__ void t_head_reduce(const float* __restrict__ hpart, int BS, float* __restrict__ ghead)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= HP_FLOATS) return;
    float s = 0.0f;
#pragma unroll 16   // (loads in flight together; the additions keep their order)
    for (int b = 0; b < BS; b++) s += hpart[(size_t)b * HP_FLOATS + i];
    int o;
    if (i < HP_PD_B) o = H_PD_W + i;
    else if (i < HP_V1_W) o = H_PD_B + (i - HP_PD_B);
    else if (i < HP_V1_B) o = H_V1_W + (i - HP_V1_W);
    else if (i < HP_V2_W) o = H_V1_B + (i - HP_V1_B);
    else if (i < HP_V2_B) o = H_V2_W + (i - HP_V2_W);
    else o = H_V2_B;
    ghead[o] = s;
}

// BN backward of the 3 head channels: dpv (dz) -> gradients of gamma/beta and dpv := d(conv output).  Two stages (sums,
// apply) so that a data-parallel step can all-reduce hsum = {s[3], sx[3]} in between; n = rows of the GLOBAL batch.
__global__ __launch_bounds__(1024) void t_head_bn_bwd_sums(const float* __restrict__ pv0, const float* __restrict__ hstat, int M,
                                                           const float* __restrict__ dpv, double* __restrict__ hsum)
{
    __shared__ double sh[1024];
    for (int ch = 0; ch < 3; ch++) {
        const float mu = hstat[ch], is = hstat[3 + ch];
        double s = 0.0, sx = 0.0;
        for (int r = threadIdx.x; r < M; r += 1024) {
            const float dz = dpv[(size_t)r * 4 + ch];
            s += dz;
            sx += (double)dz * (double)((pv0[(size_t)r * 4 + ch] - mu) * is);
        }
        s = block_sum_1024(s, sh);
        sx = block_sum_1024(sx, sh);
        if (threadIdx.x == 0) { hsum[ch] = s; hsum[3 + ch] = sx; }
    }
}
__global__ __launch_bounds__(1024) void t_head_bn_bwd(const float* __restrict__ pv0, const float* __restrict__ hp, const float* __restrict__ hstat,
                                                      int M, const double* __restrict__ hsum, float n, float gscale, float* __restrict__ dpv,
                                                      float* __restrict__ ghead)
{
    for (int ch = 0; ch < 3; ch++) {
        const float mu = hstat[ch], is = hstat[3 + ch];
        const double s = hsum[ch], sx = hsum[3 + ch];
        const int C = ch < 2 ? 2 : 1, k = ch < 2 ? ch : 0, base = ch < 2 ? H_PI_BN : H_V_BN;
        if (threadIdx.x == 0 && blockIdx.x == 0) { ghead[base + k] = (float)sx * gscale; ghead[base + C + k] = (float)s * gscale; }
        const float gamma = hp[base + k], fs = (float)s / n, fsx = (float)sx / n;
        for (int r = blockIdx.x * 1024 + threadIdx.x; r < M; r += gridDim.x * 1024) {
            const float dz = dpv[(size_t)r * 4 + ch];
            const float xh = (pv0[(size_t)r * 4 + ch] - mu) * is;
            dpv[(size_t)r * 4 + ch] = gamma * is * (dz - fs - xh * fsx);
        }
    }
}

// dH[r][c] = dp0 * pi_w[c][0] + dp1 * pi_w[c][1] + dv * v_w[c]; partial d(pi_w), d(v_w) per block of RB rows
__global__ __launch_bounds__(256) void t_head_conv_bwd(const float* __restrict__ H, const float* __restrict__ dpv, const float* __restrict__ hp,
                                                       int M, float* __restrict__ dH, float* __restrict__ part /* [R][3][256] */)
{
    const int c = threadIdx.x, r0 = blockIdx.x * RB, r1 = min(M, r0 + RB);
    const float w0 = hp[H_PI_W + c * 2], w1 = hp[H_PI_W + c * 2 + 1], w2 = hp[H_V_W + c];
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
    for (int r = r0; r < r1; r++) {
        const float4 d = reinterpret_cast<const float4*>(dpv)[r];
        const float h = H[(size_t)r * NF + c];
        dH[(size_t)r * NF + c] = d.x * w0 + d.y * w1 + d.z * w2;
        g0 += h * d.x; g1 += h * d.y; g2 += h * d.z;
    }
    part[((size_t)blockIdx.x * 3 + 0) * NF + c] = g0;
    part[((size_t)blockIdx.x * 3 + 1) * NF + c] = g1;
    part[((size_t)blockIdx.x * 3 + 2) * NF + c] = g2;
}
__global__ __launch_bounds__(256) void t_head_conv_bwd_finalize(const float* __restrict__ part, int R, float* __restrict__ ghead)
{
    const int c = threadIdx.x;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll 8
    for (int b = 0; b < R; b++) {
        g0 += part[((size_t)b * 3 + 0) * NF + c];
        g1 += part[((size_t)b * 3 + 1) * NF + c];
        g2 += part[((size_t)b * 3 + 2) * NF + c];
    }
    ghead[H_PI_W + c * 2] = g0;
    ghead[H_PI_W + c * 2 + 1] = g1;
    ghead[H_V_W + c] = g2;
}

}  // namespace
