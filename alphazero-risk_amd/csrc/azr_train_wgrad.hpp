// azr_train_wgrad.hpp — the weight gradient of a tower conv: t_wgrad_g5 (t_wgrad_rs, the older formulation, with the test hooks only) and the
// slice sum
// (A private header of azr_train.hip, the one translation unit that includes it: everything here has internal linkage.)
#pragma once
#include "azr_train_conv.hpp"

namespace {

typedef __attribute__((ext_vector_type(4))) short s16x4;

// transposed read of one MFMA operand fragment: two 4-row blocks (rows k..k+3 of the lane's group, then k+4..k+7); the
// arguments are absolute LDS addresses (no base to add), IMM a compile-time byte offset that lands in the instruction
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
template <int IMM>
__device__ __forceinline__ s16x8 lds_tr8(uint32_t a_lo, uint32_t a_hi)
{
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<lds_s16x4*>((uintptr_t)a_lo) + IMM / 8);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<lds_s16x4*>((uintptr_t)a_hi) + IMM / 8);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

#ifdef AZR_TEST_HOOKS   // the older formulation of the weight gradient: libazr_hip_test.so only (AZR_TRAIN_WGRAD=rs), what t_wgrad_g5 is compared with
// ---------------------------------------------------------------------------------------------------------------------
// t_wgrad_rs: the weight gradient  dW[tap][ci][co] = sum over rows of A[row + tap][ci] * dY[row][co]  (split bf16, 3 passes).
// The reduction runs over ROWS, the slow index of both operands ([row][channel] in memory): the MFMA wants 8 consecutive
// rows of one channel per lane.  gfx950's transposed LDS read (ds_read_b64_tr_b16) delivers exactly that from row-major
// tiles, and because every lane supplies the ADDRESS of one row of a 4-row block, the tap shift and the board-edge mask
// cost nothing: an out-of-board source row is simply the address of a zero row (no im2col, no register transposes, no masks).
//   block = ONE WAVE = one slice of whole boards (the split-K unit) x one 16-channel ci tile x 64 output channels:
//   9 taps x 4 co tiles = 36 accumulator tiles; a dY fragment feeds 9 taps, an A fragment 4 co tiles;
//   per k-step (32 rows) the wave stages its 32 rows x 64 co of dY and 46 rows (7 halo rows each side) x 16 ci of A, both
//   parts, through registers into its private LDS tile: 108 MFMAs per k-step, no barrier anywhere.
// Blocks of one slice are NS apart in blockIdx (same XCD: the slice's dY is fetched into one L2).
// ---------------------------------------------------------------------------------------------------------------------
struct Wg {
    static constexpr int KR = 32, HALO = 7, AR = KR + 2 * HALO;
    // Tile rows are placed for conflict-free transposed reads: a 32-lane half reads 4 rows r..r+3 and the 4 rows 8 further,
    // 32 bytes (8 banks) each; with a row pitch of 8 banks (mod 64) and 32 more banks in front of every further group of 8
    // rows, the eight rows cover the 64 banks once — for any tap shift of the A rows too.
    static constexpr int AST = 32;                 // bytes per row of the A tile (16 ci)
    static constexpr int APB = (AR + 1) * AST + (AR / 8) * 128;   // one part: rows and gaps, incl. the zero row (row AR)
    static constexpr int GST = 160;                // bytes per row of the dY tile (this wave's 64 co + 32 B pad: 40 banks)
    static constexpr int GPB = KR * GST + (KR / 8) * 128;
    __host__ __device__ static constexpr int arow(int r) { return r * AST + (r >> 3) * 128; }
    __host__ __device__ static constexpr int grow(int r) { return r * GST + (r >> 3) * 128; }
    static constexpr int BUF = 2 * APB + 2 * GPB;  // A part 0 | A part 1 | dY part 0 | dY part 1
    static constexpr int LDS_BYTES = BUF;          // ONE buffer: a wave's LDS operations run in program order (see t_wgrad_rs)
};
// one k-step (32 rows) of t_wgrad_rs.  With one wave per SIMD nothing hides a latency: the A fragments of tap t + 1 are
// requested BEFORE the 12 MFMAs of tap t are issued (two fragment slots, pinned with scheduling barriers — left alone, the
// compiler reuses one slot and waits for every read in front of its MFMAs), and everything else is kept to the reads
// themselves, one v_cndmask per A read (valid source row or the zero row: the row addresses are loop-invariant registers,
// part offsets are instruction immediates) and eight edge tests per k-step whose combinations per tap are scalar.
// (One loop body: two copies of the k-step in one loop made the compiler shuffle all 144 accumulators at the back-edge.)
template <int T>
__device__ __forceinline__ void wg_afrag(int y1, int x1, int y2, int x2, const uint32_t (&aoff)[9][2], uint32_t a_zero, s16x8& ah, s16x8& am)
{
    constexpr int dy = T / 3 - 1, dx = T % 3 - 1;
    const bool v1 = (dy < 0 ? y1 > 0 : dy > 0 ? y1 < 6 : true) && (dx < 0 ? x1 > 0 : dx > 0 ? x1 < 5 : true);
    const bool v2 = (dy < 0 ? y2 > 0 : dy > 0 ? y2 < 6 : true) && (dx < 0 ? x2 > 0 : dx > 0 ? x2 < 5 : true);
    const uint32_t o1 = v1 ? aoff[T][0] : a_zero, o2 = v2 ? aoff[T][1] : a_zero;
    ah = lds_tr8<0>(o1, o2);
    am = lds_tr8<Wg::APB>(o1, o2);
}
template <int T>
__device__ __forceinline__ void wg_tap(int y1, int x1, int y2, int x2, const uint32_t (&aoff)[9][2], uint32_t a_zero, const s16x8 (&gf)[2][4],
                                       s16x8 (&ah)[2], s16x8 (&am)[2], f32x4 (&acc)[9][4])
{
    if constexpr (T + 1 < 9) wg_afrag<T + 1>(y1, x1, y2, x2, aoff, a_zero, ah[(T + 1) & 1], am[(T + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < 4; c++)
        acc[T][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, am[T & 1]), __builtin_bit_cast(bf16x8, gf[0][c]), acc[T][c], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < 4; c++)
        acc[T][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ah[T & 1]), __builtin_bit_cast(bf16x8, gf[1][c]), acc[T][c], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < 4; c++)
        acc[T][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ah[T & 1]), __builtin_bit_cast(bf16x8, gf[0][c]), acc[T][c], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void wg_kstep(int& pos1, int& pos2, const uint32_t (&aoff)[9][2], uint32_t a_zero, uint32_t g_lo, uint32_t g_hi,
                                         f32x4 (&acc)[9][4])
{
    const int y1 = pos1 / 6, x1 = pos1 - 6 * y1, y2 = pos2 / 6, x2 = pos2 - 6 * y2;
    s16x8 gf[2][4];   // dY fragments [part][co tile]
    s16x8 ah[2], am[2];
    gf[0][0] = lds_tr8<0>(g_lo, g_hi); gf[0][1] = lds_tr8<32>(g_lo, g_hi); gf[0][2] = lds_tr8<64>(g_lo, g_hi); gf[0][3] = lds_tr8<96>(g_lo, g_hi);
    wg_afrag<0>(y1, x1, y2, x2, aoff, a_zero, ah[0], am[0]);
    gf[1][0] = lds_tr8<Wg::GPB>(g_lo, g_hi); gf[1][1] = lds_tr8<Wg::GPB + 32>(g_lo, g_hi);
    gf[1][2] = lds_tr8<Wg::GPB + 64>(g_lo, g_hi); gf[1][3] = lds_tr8<Wg::GPB + 96>(g_lo, g_hi);
    wg_tap<0>(y1, x1, y2, x2, aoff, a_zero, gf, ah, am, acc);
    wg_tap<1>(y1, x1, y2, x2, aoff, a_zero, gf, ah, am, acc);
    wg_tap<2>(y1, x1, y2, x2, aoff, a_zero, gf, ah, am, acc);
    wg_tap<3>(y1, x1, y2, x2, aoff, a_zero, gf, ah, am, acc);
    wg_tap<4>(y1, x1, y2, x2, aoff, a_zero, gf, ah, am, acc);
    wg_tap<5>(y1, x1, y2, x2, aoff, a_zero, gf, ah, am, acc);
    wg_tap<6>(y1, x1, y2, x2, aoff, a_zero, gf, ah, am, acc);
    wg_tap<7>(y1, x1, y2, x2, aoff, a_zero, gf, ah, am, acc);
    wg_tap<8>(y1, x1, y2, x2, aoff, a_zero, gf, ah, am, acc);
    pos1 += Wg::KR; if (pos1 >= NPOS) pos1 -= NPOS;
    pos2 += Wg::KR; if (pos2 >= NPOS) pos2 -= NPOS;
}

// One WAVE per block: a wave's tiles (its 64 co columns of dY, its own copy of the 16-ci A rows) are private, so there is
// nothing to synchronise with — no barrier, and the four waves of a CU (four blocks, 15 KB of LDS each) drift apart and hide
// each other's bubbles.  A single LDS buffer suffices: the next tile travels global -> registers while this k-step
// computes and is stored over the current one AFTER the k-step's last fragment read has been issued — the LDS operations
// of one wave execute in program order.  Measured per k-step on one box (rocprofv3 kernel time, parts removed): the 108
// MFMAs 37 us of the 67, the staging 10, the A fragment reads 7: with one wave per SIMD nothing overlaps for free.
__global__ __launch_bounds__(64, 1) void t_wgrad_rs(Parts A, Parts G, float* __restrict__ out, int M, int NS, int rows_per_slice)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t wg_lds[];
    const int lane = threadIdx.x;
    const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
    const int slice = blockIdx.x % NS, rest = blockIdx.x / NS, cit = rest & 15, wq = rest >> 4;   // wq = which 64 co columns
    const int rbeg = slice * rows_per_slice, rend = min(M, rbeg + rows_per_slice);
    const int nks = (rend - rbeg + Wg::KR - 1) / Wg::KR;   // k-steps; a slice that is not a multiple of 32 rows (8 boards = 10.5 k-steps) ends
                                                          // inside one: the dY rows past the slice read as zero (range of gsrc below)

    // zero rows of the two A parts
    if (lane < 2 * (Wg::AST / 4))
        reinterpret_cast<uint32_t*>(wg_lds + (lane / (Wg::AST / 4)) * Wg::APB + Wg::arow(Wg::AR))[lane % (Wg::AST / 4)] = 0u;

    // staging units of this lane: 8 of the dY tile (4 (row, 16-byte segment) pairs x 2 parts: always inside the slice) and
    // up to 4 of the A tile (2 per part; halo rows before row 0 or after row M - 1 are out of range of the buffer resource
    // and read as 0).  Buffer loads: the k-step advances a scalar offset.
    const __amdgpu_buffer_rsrc_t gsrc0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(G.p[0]), (short)0, rend * NF * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t gsrc1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(G.p[1]), (short)0, rend * NF * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t asrc0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(A.p[0]), (short)0, M * NF * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t asrc1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(A.p[1]), (short)0, M * NF * 2, 0x00020000);
    uint32_t goffs[4], gl[4], aoffs[2], al[2];
    bool a_unit[2];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = i * 8 + (lane >> 3), seg = lane & 7;
        goffs[i] = (uint32_t)((rbeg + row) * NF + wq * 64 + seg * 8) * 2u;
        gl[i] = (uint32_t)(2 * Wg::APB + Wg::grow(row) + seg * 16);
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int v = lane + 64 * j, row = v >> 1, seg = v & 1;
        a_unit[j] = v < 2 * Wg::AR;
        // (as a vector offset, so that the range check sees it: rows before 0 wrap to huge offsets, rows past M - 1 exceed M * 512)
        aoffs[j] = a_unit[j] ? (uint32_t)(((rbeg - Wg::HALO + row) * NF + cit * 16 + seg * 8) * 2) : 0xfffffff0u;
        al[j] = (uint32_t)(Wg::arow(a_unit[j] ? row : Wg::AR - 1) + seg * 16);
    }
    u32x4 sg[8], sa[4];
    auto fetch = [&](int ks) {
        const int so = ks * (Wg::KR * NF * 2);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            sg[i] = __builtin_amdgcn_raw_buffer_load_b128(gsrc0, goffs[i], so, 0);
            sg[i + 4] = __builtin_amdgcn_raw_buffer_load_b128(gsrc1, goffs[i], so, 0);
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t vo = a_unit[j] ? aoffs[j] + (uint32_t)so : 0xfffffff0u;
            sa[j] = __builtin_amdgcn_raw_buffer_load_b128(asrc0, vo, 0, 0);
            sa[j + 2] = __builtin_amdgcn_raw_buffer_load_b128(asrc1, vo, 0, 0);
        }
    };
    auto stash = [&]() {
        uint8_t* b = wg_lds;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            *reinterpret_cast<u32x4*>(b + gl[i]) = sg[i];
            *reinterpret_cast<u32x4*>(b + Wg::GPB + gl[i]) = sg[i + 4];
        }
#pragma unroll
        for (int j = 0; j < 2; j++)
            if (a_unit[j]) {
                *reinterpret_cast<u32x4*>(b + al[j]) = sa[j];
                *reinterpret_cast<u32x4*>(b + Wg::APB + al[j]) = sa[j + 2];
            }
    };
    fetch(0);
    stash();

    f32x4 acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; t++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the two tile rows this lane addresses in a transposed read: k1 = 8g + q and k1 + 4; their board cells and, per tap, the
    // LDS addresses of their source rows (loop-invariant: the tile moves, the lane's place in it does not)
    const int k1 = 8 * g + q;
    int pos1 = k1 % NPOS, pos2 = (k1 + 4) % NPOS;      // (slices start on a board boundary)
    const uint32_t lbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)wg_lds;   // absolute LDS addresses
    uint32_t aoff[9][2];
#pragma unroll
    for (int t = 0; t < 9; t++) {
        const int sh = Wg::HALO + (t / 3 - 1) * 6 + (t % 3 - 1);   // source tile row = k + sh
        aoff[t][0] = lbase + (uint32_t)(Wg::arow(k1 + sh) + p * 8);
        aoff[t][1] = lbase + (uint32_t)(Wg::arow(k1 + 4 + sh) + p * 8);
    }
    const uint32_t a_zero = lbase + (uint32_t)(Wg::arow(Wg::AR) + p * 8);
    const uint32_t g_lo = lbase + (uint32_t)(2 * Wg::APB + Wg::grow(k1) + p * 8);
    const uint32_t g_hi = lbase + (uint32_t)(2 * Wg::APB + Wg::grow(k1 + 4) + p * 8);

    for (int ks = 0; ks < nks; ks++) {
        if (ks + 1 < nks) fetch(ks + 1);
        asm volatile("" ::: "memory");   // (the fragment reads below follow this wave's own tile stores in program order ...
        wg_kstep(pos1, pos2, aoff, a_zero, g_lo, g_hi, acc);
        asm volatile("" ::: "memory");   //  ... and the stores of the next tile follow the reads)
        if (ks + 1 < nks) stash();
    }
    float* o = out + (size_t)slice * KC * NF;
#pragma unroll
    for (int t = 0; t < 9; t++)
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int e = 0; e < 4; e++)
                o[(size_t)(t * NF + cit * 16 + 4 * g + e) * NF + wq * 64 + c * 16 + i16] = acc[t][c][e];
}
#endif   // AZR_TEST_HOOKS

// ---------------------------------------------------------------------------------------------------------------------
// t_wgrad_g5: the same weight gradient with the reduction index laid out so that the 3 x 3 taps share operand fragments.
// t_wgrad_rs reduces over rows in memory order: every tap is its own shift of the A rows, so a k-step reads 9 x 2 A fragments from LDS
// for 108 MFMAs, and its 52 transposed reads per wave (4 waves per CU) hold the matrix pipe at one half.  Here a k-step is ONE BOARD ROW
// y OF FIVE BOARDS: k = 6 j + x (board j of the group, column x; k = 30, 31 are zero).  Then
//   * the dy shift of a tap is a shift by whole k-steps: the A fragments of board row y + dy are those read for k-step y + dy — a
//     fragment is read from LDS ONCE and serves three k-steps out of a ring of three rows in registers (3 dx x 2 parts x 3 rows);
//   * the dx shift is the lane's source-row address, loop-invariant (x = k mod 6 belongs to the lane): no edge tests in the loop;
//   * taps that leave the board vertically are whole k-steps of zeros and are skipped (y = 0: dy = -1, y = 6: dy = +1): 57 of 63
//     tap-rows per group, which pays for the 2 idle k of 32;
//   * per k-step 12 A reads + 16 dY reads instead of 36 + 16, 10 KB of tile stores instead of 12, no halo rows.
// The k-steps of a slice form one flat sequence s (7 per group of 5 boards; "row 7" of a group is row 0 of the next, and the taps that
// would mix them are the skipped ones).  In k-step s the LDS tile holds {dY(s + 1), A(s + 2)}: stored at the start of the k-step (its
// global loads were issued one k-step earlier), read into the NEXT fragment registers while this k-step's MFMAs run from registers —
// the dY fragments at once, the A fragments into the ring slot of row s - 1 once that row's taps (dy = -1) are done.  Ring slots and
// the dY double buffer are compile-time: the loop body is six k-steps.
// Measured (batch 512, one box, rocprofv3 averages over 1000 launches; profiles/r04_train_step.txt): 62.2 us against 68.9 for t_wgrad_rs
// (64.3 before the memory operations were dealt between the MFMAs).  Of the 62: 39 are the 4788 MFMAs of a block (7 groups x 7 k-steps),
// ~9 the 35 MB of split-K partials that all 960 waves write at the same moment, ~3 the prologue's three dependent round trips.
// ---------------------------------------------------------------------------------------------------------------------
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}
template <int NC>   // NC = co tiles of 16 per wave: 4 (64 output channels, 64 blocks per slice) or 2 (32 channels, 128 blocks per slice)
struct Wg5 {
    static constexpr int GB = 5, KR = 32, ROWS_Y = 7;
    static constexpr int AST = 32;                                     // bytes per row of the A tile (16 ci)
    __host__ __device__ static constexpr int arow(int r) { return r * AST + (r >> 3) * 128; }   // rows 0 .. 31, row 32 = the zero row
    static constexpr int APB = 33 * AST + 5 * 128;
    // dY tile rows: NC x 32 bytes + pad so that the pitch is 8 banks mod 16 — with 32 banks in front of every further group of 8 rows the
    // eight rows of a transposed read (r .. r + 3 and r + 8 .. r + 11, 8 banks each) cover the 64 banks once (40 banks / 24 banks)
    static constexpr int GST = NC == 4 ? 160 : 96;
    __host__ __device__ static constexpr int grow(int r) { return r * GST + (r >> 3) * 128; }
    static constexpr int GPB = KR * GST + (KR / 8) * 128;
    static constexpr int LDS_BYTES = 2 * APB + 2 * GPB;               // one wave's tile: A part 0 | A part 1 | dY part 0 | dY part 1
    static constexpr int LDS_BLOCK = 4 * LDS_BYTES > 2 * 9 * NC * 1024 ? 4 * LDS_BYTES : 2 * 9 * NC * 1024;   // four waves' tiles, or two accumulator sets in the closing sum
    static constexpr int COW = 16 * NC;                                // output channels per wave
    static constexpr int BLOCKS_PER_SLICE = 16 * (NF / COW);
    // the memory operations of a k-step, in dependence order: tile stores (GU dY units x 2 parts, 2 A units), global loads (the same
    // units), dY fragments (2 parts x NC, two reads each), A fragments (3 dx x 2 parts, two reads each)
    static constexpr int GU = NC;                                      // 16-byte dY units per lane and part (32 rows x 2 NC segments / 64 lanes)
    static constexpr int NW = 2 * GU + 2, NL = 2 * GU + 2, NG = 2 * NC, NA = 6, NOPS = NW + NL + NG + NA;
    static constexpr int BUDGET = NC == 4 ? 6 : 4;                     // memory instructions dealt into one tap's slot (3 NC MFMAs)
    __host__ __device__ static constexpr int cost(int k) { return k < NW + NL ? 1 : 2; }
    __host__ __device__ static constexpr int slot_lo(int slot)          // first operation of a slot: greedy fill in order
    {
        int k = 0;
        for (int sl = 0; sl < slot; sl++) {
            int b = 0;
            while (k < NOPS && b + cost(k) <= BUDGET) { b += cost(k); k++; }
        }
        return k;
    }
    static_assert(slot_lo(9) == NOPS, "nine slots take every operation");
    static_assert(slot_lo(3) <= NW + NL + NG, "the A fragment reads stand behind the dy = -1 taps (slots 0 - 2)");
};

template <int T, int NC>
__device__ __forceinline__ void g5_tap(const s16x8 (&a)[2], const s16x8 (&gf)[2][NC], f32x4 (&acc)[9][NC])
{
#pragma unroll
    for (int c = 0; c < NC; c++)
        acc[T][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[1]), __builtin_bit_cast(bf16x8, gf[0][c]), acc[T][c], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < NC; c++)
        acc[T][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[0]), __builtin_bit_cast(bf16x8, gf[1][c]), acc[T][c], 0, 0, 0);
#pragma unroll
    for (int c = 0; c < NC; c++)
        acc[T][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[0]), __builtin_bit_cast(bf16x8, gf[0][c]), acc[T][c], 0, 0, 0);
}

// A block is FOUR waves = four slices of one (ci tile, co range): each wave runs its slice alone (private tile, no barrier in the loop),
// and the four accumulator sets are summed through LDS before anything is written — a quarter of the split-K partials leave the chip and
// come back into the slice sum (512 records: 4 instead of 15 per weight; t_sum_slices_fin 10.6 -> 6.4 us, the kernel itself unchanged:
// the two rounds through LDS cost what the smaller write saves).  Block id -> (quad of slices, rest): the blocks of a quad are NQ apart,
// i.e. on the same two XCDs, whose L2s then hold that quad's dY.
template <int NC>
__global__ __launch_bounds__(256, 1) void t_wgrad_g5(Parts A, Parts G, float* __restrict__ out, int boards, int NS, int boards_per_slice)
{
    using W = Wg5<NC>;
    extern __shared__ __attribute__((aligned(16))) uint8_t wg_lds_all[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;   // (uniform by construction: say so, or every buffer load gets a waterfall loop around its descriptor)
    uint8_t* wg_lds = wg_lds_all + wave * W::LDS_BYTES;
    const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
    const int NQ = (NS + 3) / 4;
    const int quad = blockIdx.x % NQ, rest = blockIdx.x / NQ, cit = rest & 15, wq = rest >> 4;   // wq = which COW output channels
    const int slice = quad * 4 + wave;
    const int bbeg = slice * boards_per_slice, bend = min(boards, bbeg + boards_per_slice);
    const int S = slice < NS ? W::ROWS_Y * ((bend - bbeg + W::GB - 1) / W::GB) : 0;   // k-steps of the slice (a quad past the last slice: none)

    if (lane < 2 * (W::AST / 4))   // zero rows of the two A parts
        reinterpret_cast<uint32_t*>(wg_lds + (lane / (W::AST / 4)) * W::APB + W::arow(32))[lane % (W::AST / 4)] = 0u;

    // Staging units of this lane: GU of the dY tile per part ((tile row, 16-byte segment) pairs) and one of the A tile per part.
    // Tile row k = board 6 j + column x of the group; rows 30, 31 and the boards past the slice are out of range of the buffer resources
    // (everything is in the vector offset, which the range check sees) and arrive as zeros.
    const uint32_t range = (uint32_t)bend * NPOS * NF * 2u;
    const __amdgpu_buffer_rsrc_t gsrc0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(G.p[0]), (short)0, range, 0x00020000);
    const __amdgpu_buffer_rsrc_t gsrc1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(G.p[1]), (short)0, range, 0x00020000);
    const __amdgpu_buffer_rsrc_t asrc0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(A.p[0]), (short)0, range, 0x00020000);
    const __amdgpu_buffer_rsrc_t asrc1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(A.p[1]), (short)0, range, 0x00020000);
    constexpr uint32_t OOR = 0xfffffff0u;
    constexpr int SEGS = 2 * NC;   // 16-byte segments of a dY tile row
    uint32_t gvo[W::GU], gl[W::GU], avo, al;
#pragma unroll
    for (int i = 0; i < W::GU; i++) {
        const int u = lane + 64 * i, k = u / SEGS, seg = u % SEGS;
        gvo[i] = k < 30 ? (uint32_t)((((bbeg + k / 6) * NPOS + k % 6) * NF + wq * W::COW + seg * 8) * 2) : OOR;
        gl[i] = (uint32_t)(2 * W::APB + W::grow(k) + seg * 16);
    }
    {
        const int k = lane >> 1, seg = lane & 1;
        avo = k < 30 ? (uint32_t)((((bbeg + k / 6) * NPOS + k % 6) * NF + cit * 16 + seg * 8) * 2) : OOR;
        al = (uint32_t)(W::arow(k) + seg * 16);
    }
    // byte offset of flat k-step s: group s / 7 (5 boards further each), board row s % 7
    auto step_off = [](int s) -> uint32_t { return (uint32_t)(((s / W::ROWS_Y) * W::GB * NPOS + (s % W::ROWS_Y) * 6) * NF * 2); };
    u32x4 sg[2 * W::GU], sa[2];

    // the two tile rows this lane addresses in a transposed read (k1 = 8 g + q and k1 + 4), their columns, and per dx the LDS address of
    // the source row: k + dx inside the board row, the zero row outside it (and for the idle k = 30, 31)
    const int k1 = 8 * g + q, k2 = k1 + 4;
    const uint32_t lbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)wg_lds;
    const uint32_t a_zero = lbase + (uint32_t)(W::arow(32) + p * 8);
    uint32_t aoff[3][2];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const int x1 = k1 % 6 + d - 1, x2 = k2 % 6 + d - 1;
        aoff[d][0] = (k1 < 30 && x1 >= 0 && x1 < 6) ? lbase + (uint32_t)(W::arow(k1 + d - 1) + p * 8) : a_zero;
        aoff[d][1] = (k2 < 30 && x2 >= 0 && x2 < 6) ? lbase + (uint32_t)(W::arow(k2 + d - 1) + p * 8) : a_zero;
    }
    const uint32_t g_lo = lbase + (uint32_t)(2 * W::APB + W::grow(k1) + p * 8);
    const uint32_t g_hi = lbase + (uint32_t)(2 * W::APB + W::grow(k2) + p * 8);

    f32x4 acc[9][NC];
#pragma unroll
    for (int t = 0; t < 9; t++)
#pragma unroll
        for (int c = 0; c < NC; c++) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    s16x8 R[3][3][2];     // A fragments [ring slot = board-row index mod 3][dx][part]
    s16x8 gf[2][2][NC];   // dY fragments [k-step mod 2][part][co tile]

    // Operation K of a k-step that stores tile TS + 1, requests tile TS + 2 (vg, va: its vector offsets), reads the dY fragments into gf[GN]
    // and the A fragments into ring slot RM:  tile stores | global loads | dY fragments | A fragments (Wg5: NW, NL, NG, NA)
    uint32_t vg[W::GU], va = OOR;
    auto op = [&](auto kk, auto gnn, auto rmm) {
        constexpr int K = decltype(kk)::value, GN = decltype(gnn)::value, RM = decltype(rmm)::value;
        constexpr int KW = K, KL = K - W::NW, KG = K - W::NW - W::NL, KA = K - W::NW - W::NL - W::NG;
        if constexpr (KW < W::GU) *reinterpret_cast<u32x4*>(wg_lds + gl[KW]) = sg[KW];
        else if constexpr (KW < 2 * W::GU) *reinterpret_cast<u32x4*>(wg_lds + W::GPB + gl[KW - W::GU]) = sg[KW];
        else if constexpr (KW == 2 * W::GU) *reinterpret_cast<u32x4*>(wg_lds + al) = sa[0];
        else if constexpr (KW == 2 * W::GU + 1) *reinterpret_cast<u32x4*>(wg_lds + W::APB + al) = sa[1];
        else if constexpr (KL < W::GU) sg[KL] = __builtin_amdgcn_raw_buffer_load_b128(gsrc0, vg[KL], 0, 0);
        else if constexpr (KL < 2 * W::GU) sg[KL] = __builtin_amdgcn_raw_buffer_load_b128(gsrc1, vg[KL - W::GU], 0, 0);
        else if constexpr (KL == 2 * W::GU) sa[0] = __builtin_amdgcn_raw_buffer_load_b128(asrc0, va, 0, 0);
        else if constexpr (KL == 2 * W::GU + 1) sa[1] = __builtin_amdgcn_raw_buffer_load_b128(asrc1, va, 0, 0);
        else if constexpr (KG < W::NG) gf[GN][KG / NC][KG % NC] = lds_tr8<(KG / NC) * W::GPB + (KG % NC) * 32>(g_lo, g_hi);
        else R[RM][KA / 2][KA % 2] = lds_tr8<(KA % 2) * W::APB>(aoff[KA / 2][0], aoff[KA / 2][1]);
    };
    auto offsets = [&](int sd, int sa_) {   // vector offsets of the loads of {dY(sd), A(sa_)}
        const uint32_t so_g = step_off(sd), so_a = step_off(sa_);
#pragma unroll
        for (int i = 0; i < W::GU; i++) vg[i] = gvo[i] == OOR ? OOR : gvo[i] + so_g;
        va = avo == OOR ? OOR : avo + so_a;
    };
#define IC(n) std::integral_constant<int, (n)>{}
    // prologue: A(0) -> ring slot 0; tile 0 = {dY(0), A(1)} -> gf[0], ring slot 1; tile 1 on its way
    offsets(0, 0);
    op(IC(W::NW + 2 * W::GU), IC(0), IC(0)); op(IC(W::NW + 2 * W::GU + 1), IC(0), IC(0));                   // load A(0)
    op(IC(2 * W::GU), IC(0), IC(0)); op(IC(2 * W::GU + 1), IC(0), IC(0));                                   // store it
    asm volatile("" ::: "memory");
    static_for<W::NW + W::NL + W::NG, W::NOPS>([&](auto k) { op(k, IC(0), IC(0)); });                       // -> R[0]
    offsets(0, 1);
    static_for<W::NW, W::NW + W::NL>([&](auto k) { op(k, IC(0), IC(0)); });                                 // load tile 0
    asm volatile("" ::: "memory");
    static_for<0, W::NW>([&](auto k) { op(k, IC(0), IC(0)); });                                             // store it
    asm volatile("" ::: "memory");
    static_for<W::NW + W::NL, W::NOPS>([&](auto k) { op(k, IC(0), IC(1)); });                               // -> gf[0], R[1]
    offsets(1, 2);
    static_for<W::NW, W::NW + W::NL>([&](auto k) { op(k, IC(0), IC(0)); });                                 // load tile 1

    // One k-step = one straight-line piece of code per ring phase, cut into SLOTS of one tap (3 NC MFMAs) each.  The memory instructions of
    // the k-step are dealt over the slots in dependence order (Wg5::slot_lo) and inside a slot one is issued behind each of the first MFMAs
    // (sched_group_barrier; a slot is one scheduling region): a lone wave issues in order, and ten stores or sixteen reads in a row in
    // front of the MFMAs leave the matrix pipe idle for as long as they take to issue.
    int y = 0;
    auto kstep = [&](auto ph, int s) {
        constexpr int PH = decltype(ph)::value;
        constexpr int rm = (PH + 2) % 3, r0 = PH % 3, rp = (PH + 1) % 3, gc = PH % 2, gn = (PH + 1) % 2;
        offsets(s + 2, s + 3);   // tile s + 2 = {dY(s + 2), A(s + 3)} (past the slice: zeros or the next slice's rows — nobody multiplies them)
        auto slot = [&](auto tt) {
            constexpr int T = decltype(tt)::value, LO = W::slot_lo(T), HI = W::slot_lo(T + 1);
            constexpr int NI = []() { int n = 0; for (int k = LO; k < HI; k++) n += W::cost(k); return n; }();
            constexpr int RS = T / 3 == 0 ? rm : T / 3 == 1 ? r0 : rp;
            auto ops = [&](auto k) { op(k, IC(gn), IC(rm)); };   // (the A fragments: A(s + 2) into the slot row s - 1 has left)
            __builtin_amdgcn_sched_barrier(0);
            // (the taps that leave the board vertically are whole k-steps of zeros: skipped; their slots' memory operations are not)
            if (T / 3 == 1 || (T / 3 == 0 ? y > 0 : y < W::ROWS_Y - 1)) {
                static_for<LO, HI>(ops);
                g5_tap<T, NC>(R[RS][T % 3], gf[gc], acc);
#pragma unroll
                for (int i = 0; i < NI; i++) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA
                    __builtin_amdgcn_sched_group_barrier(0x0a0, 1, 0);   // one LDS or global-load instruction
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 3 * NC - NI, 0);
            } else {
                asm volatile("; slot without its tap" ::: "memory");   // (keeps the two branches' common operations from being hoisted in front of the branch)
                static_for<LO, HI>(ops);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        static_for<0, 9>(slot);
        y = y == W::ROWS_Y - 1 ? 0 : y + 1;
    };
    for (int s = 0; s < S; s += 6) {
        kstep(IC(0), s);
        if (s + 1 < S) kstep(IC(1), s + 1);
        if (s + 2 < S) kstep(IC(2), s + 2);
        if (s + 3 < S) kstep(IC(3), s + 3);
        if (s + 4 < S) kstep(IC(4), s + 4);
        if (s + 5 < S) kstep(IC(5), s + 5);
    }
#undef IC
    // (w0 + w2) + (w1 + w3): two rounds through LDS (the tiles are dead behind the first barrier), 16 bytes per lane and accumulator tile
    f32x4* red = reinterpret_cast<f32x4*>(wg_lds_all) + lane;
    constexpr int TILES = 9 * NC;
    __syncthreads();
    if (wave >= 2) {
#pragma unroll
        for (int t = 0; t < 9; t++)
#pragma unroll
            for (int c = 0; c < NC; c++) red[((wave - 2) * TILES + t * NC + c) * 64] = acc[t][c];
    }
    __syncthreads();
    if (wave < 2) {
#pragma unroll
        for (int t = 0; t < 9; t++)
#pragma unroll
            for (int c = 0; c < NC; c++) acc[t][c] += red[(wave * TILES + t * NC + c) * 64];
    }
    __syncthreads();
    if (wave == 1) {
#pragma unroll
        for (int t = 0; t < 9; t++)
#pragma unroll
            for (int c = 0; c < NC; c++) red[(t * NC + c) * 64] = acc[t][c];
    }
    __syncthreads();
    if (wave != 0) return;
    float* o = out + (size_t)quad * KC * NF;
#pragma unroll
    for (int t = 0; t < 9; t++)
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const f32x4 v = acc[t][c] + red[(t * NC + c) * 64];
#pragma unroll
            for (int e = 0; e < 4; e++) o[(size_t)(t * NF + cit * 16 + 4 * g + e) * NF + wq * W::COW + c * 16 + i16] = v[e];
        }
}

// out[i] = sum_z part[z][i]
__global__ void t_sum_slices(const float* __restrict__ part, int nz, size_t n, float* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    for (int z = 0; z < nz; z++) s += part[(size_t)z * n + i];
    out[i] = s;
}

}  // namespace
