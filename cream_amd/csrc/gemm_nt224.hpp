// gemm_nt224.hpp — the 256 x 224 NT tile on v_mfma_f32_16x16x32_bf16 (gfx950) for the outputs that are a multiple of 224 wide
// (the embedding width 448 of supernet-S: proj, fc2, the fc1 / qkv / proj input gradients; qkv forward at 7 heads, N = 1344).
//
// Reference semantics: as gemm_mfma.hpp — LinearSuper.forward / qkv_super.forward = F.linear on the active block of the super
// weight (AutoFormer/model/module/Linear_super.py:38-54, qkv_super.py:45-55) and the input gradients autograd derives.
//     C(M x N) = A(M x K) . B(N x K)^T (+ bias)      both operands K-contiguous, bf16, fp32 accumulate, bf16 result
//
// Why its own kernel: 224 = 7 x 32 columns do not split over two wave columns of 32 x 32 MFMA blocks (8 x 1 waves
// spill 98 registers, 4 + 3 blocks per wave column leave 84 B of scratch and an unbalanced wave map).  224 = 14 x 16 does:
//   * 512 threads = 4 (m) x 2 (n) waves, wave tile 64 x 112 = 4 x 7 blocks of 16 x 16 = 112 accumulator registers;
//   * K-tile 64 = two 32-deep sub-steps; per sub-step a wave reads 4 + 7 fragments for 28 MFMAs.  The A fragments of both
//     sub-steps are kept, the B fragments stream in units of two, one unit ahead of the 8 MFMAs that use them (pinned
//     with sched_group_barrier): 16 + 16 + 16 fragment registers live instead of 88;
//   * staging, LDS image and swizzle are those of the two-stage gemm_nt_kernel: global -> LDS directly in 1-KB pieces of 8 rows,
//     [row][8 chunks of 16 B] with the SOURCE chunk XOR (row >> 1) & 7, two stages of (256 + 224) x 64 x 2 B = 120 KB, one
//     persistent workgroup per CU, the first K-step of the next tile requested before the epilogue of the current one;
//   * the same image is conflict-free for the 16x16x32 operand read (lane l: row l & 15, chunk 4 ks + (l >> 4)): the four
//     ds_read_b128 lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (+ 32) each take rows 0 .. 15 once — eight of them at
//     chunk c, eight at c ^ 1 — and (r & 1) * 8 + (chunk ^ (r >> 1)) runs over all sixteen 16-B slots of the 256-B bank row:
//     rows {0-3, 12-15} give c ^ {0, 1, 6, 7}, rows {4-11} give c ^ 1 ^ {2, 3, 4, 5} = c ^ {3, 2, 5, 4};
//   * swapped product D^T = B_tile . A_tile^T: a lane owns output row l & 15 and the 4 columns 4 (l >> 4) .. + 3 of a block, so
//     the accumulators leave through the LDS of stage 1 as fp32 with 16-byte writes in four passes of 64 rows (chunk positions
//     XOR row & 7: 8 consecutive lanes of a ds_write_b128 group hit 8 distinct 16-B slots of the 128-B write bank row), and
//     the epilogue stores (row, 8 columns) chunks: 16 bytes, non-temporal.
// Epilogues: plain store and + bias.  Segment addressing (nseg / kseg), the zero-filled K tail, rows beyond M and columns
// beyond N as in gemm_nt_kernel.  M arbitrary, N % 8 == 0, K % 8 == 0.
//
// Numerics: the 16x16x32 instruction adds 32 contraction elements per issue where every other tile adds 16, so on general
// operands a result may differ from the other tiles' in the last bf16 place (exact operands: bit-identical).
#pragma once
#include "gemm_mfma.hpp"

namespace cream {
namespace gemm {

constexpr int NT224_BM = 256, NT224_BN = 224;
constexpr int NT224_LDS_BYTES = nt_lds_bytes(NT224_BM, NT224_BN, 2);

template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm_nt224_kernel(const NtParams p)
{
    static_assert(EPI == EPI_STORE || EPI == EPI_BIAS, "plain and bias epilogues only");
    constexpr int BM = NT224_BM, BN = NT224_BN, BK = 64;
    constexpr int WN = 2, NW = 8, NT = NW * 64;
    constexpr int WTM = 64, WTN = 112, TM = WTM / 16, TN = WTN / 16;    // wave tile: 4 x 7 blocks of 16 x 16
    constexpr int STAGE = (BM + BN) * BK;                       // bf16 elements per stage
    constexpr int PIECES = (BM + BN) / 8;                       // 1-KB pieces (8 rows) per stage: 32 of A, 28 of B
    constexpr int NPIECE = (PIECES + NW - 1) / NW;              // per wave; the last one only for waves < PIECES % NW
    constexpr int APIECE = BM / 8 / NW;                         // pieces wave + NW i, i < APIECE, hold A rows
    constexpr int NCH = BN / 4;                                 // 4-float chunks per epilogue row
    constexpr int HM = 64, NPASS = BM / HM;                     // the epilogue takes one wave row per pass through stage 1
    static_assert(PIECES % NW != 0 && HM == WTM && HM * BN * 4 <= STAGE * 2, "tile");
    char* const smem = LdsBlock<NT224_LDS_BYTES>::get();
    uint16_t* const lds = reinterpret_cast<uint16_t*>(smem);
    float* const ctile = reinterpret_cast<float*>(smem + STAGE * 2);           // stage 1

    const int tid = threadIdx.x, lane = tid & 63, q = lane >> 4, l15 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int ntn = (p.N + BN - 1) / BN, ntiles = ntn * ((p.M + BM - 1) / BM);
    const int K = p.K;

    // ---- per-lane sources of this wave's pieces (row + this lane's k-chunk; the K offset moves per step).  The pieces of a
    //      wave are 64 rows apart: one swizzle term, one k-chunk for all of them
    const int prow = wave * 8 + (lane >> 3);
    const int cch = ((lane & 7) ^ ((prow >> 1) & 7)) * 8;
    auto sources = [&](const uint16_t* (&src)[NPIECE], int m0, int n0) {
#pragma unroll
        for (int i = 0; i < NPIECE; ++i) {
            const int row = prow + NW * 8 * i;
            if (i < APIECE) {
                src[i] = p.A + (int64_t)min(m0 + row, p.M - 1) * p.lda + cch;
            } else {
                const int n = min(n0 + min(row - BM, BN - 1), p.N - 1);    // (ragged last piece: past the tile, never issued)
                const int seg = (n >= p.nseg) + (n >= 2 * p.nseg);  // at most 3 row segments (q | k | v): no division
                src[i] = p.B + seg * p.nseg_stride + (int64_t)(n - seg * p.nseg) * p.ldb + cch;
            }
        }
    };
    // TAIL: the last K-step of a K that is no multiple of 64 — chunks beyond K re-read the last valid chunk (their products
    // are zeroed in `step`), so no load leaves the row.  kb: wave-uniform K offset of the B operand (contraction segments)
    int64_t kb = 0;
    int kin = 0;
    auto issue = [&](const uint16_t* const (&src)[NPIECE], int k0, int buf, auto tail) {
#pragma unroll
        for (int i = 0; i < NPIECE; ++i) {
            if (i == NPIECE - 1 && wave + NW * i >= PIECES) continue;          // (wave-uniform)
            const uint16_t* s = src[i] + (i < APIECE ? (int64_t)k0 : kb);
            if constexpr (decltype(tail)::value) s += min(0, K - 8 - (k0 + cch));
            __builtin_amdgcn_global_load_lds(
                s, reinterpret_cast<__attribute__((address_space(3))) void*>(
                       reinterpret_cast<uintptr_t>(lds + buf * STAGE + (wave + NW * i) * 8 * BK)), 16, 0, 0);
        }
        kb += BK;
        kin += BK;
        if (kin >= p.kseg) { kin = 0; kb += p.kseg_stride - p.kseg; }
    };
    const int sw = l15 >> 1;                                    // (row >> 1) & 7 of a row 16 j + l15
    auto frag = [&](const uint16_t* tile, int row, int chunk) -> bf16x8 {
        return *reinterpret_cast<const bf16x8*>(tile + row * BK + ((chunk ^ sw) << 3));
    };

    f32x4v acc[TN][TM];

    // one K-step from stage `buf`; vc = valid 8-wide chunks (8 unless TAIL)
    auto step = [&](int buf, int vc, auto tail) {
        constexpr bool T = decltype(tail)::value;
        const uint16_t* At = lds + buf * STAGE + (wm * WTM + l15) * BK;
        const uint16_t* Bt = lds + buf * STAGE + (BM + wn * WTN + l15) * BK;
        const bf16x8 zero = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        bf16x8 fa[2][TM], fb[2 * TN];                           // fb[7 ks + tn]
        // (the tail reads every fragment and selects, and multiplies both sub-steps — the one beyond K on zeros: no branch
        //  around an LDS read or between the MFMAs, one basic block, the same pinned schedule as a full step)
        auto ra = [&](int ks, int i) {
            fa[ks][i] = frag(At, i * 16, ks * 4 + q);
            if (T && ks * 4 + q >= vc) fa[ks][i] = zero;
        };
        auto rb = [&](int j) {
            const int ks = j / TN;
            fb[j] = frag(Bt, (j % TN) * 16, ks * 4 + q);
            if (T && ks * 4 + q >= vc) fb[j] = zero;
        };
        // program order of the reads = the order the schedule below takes them in: units of two B fragments (8 MFMAs), read
        // one unit ahead; the A fragments of the second sub-step ride with units 2 and 3
#pragma unroll
        for (int i = 0; i < TM; ++i) ra(0, i);
#pragma unroll
        for (int j = 0; j < 2 * TN; ++j) {
            rb(j);
            if (j == 5) { ra(1, 0); ra(1, 1); }
            if (j == 7) { ra(1, 2); ra(1, 3); }
        }
#pragma unroll
        for (int j = 0; j < 2 * TN; ++j) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
                acc[j % TN][tm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[j / TN][tm], acc[j % TN][tm], 0, 0, 0);
        }
        {
            // the compiler waits for LDS reads with lgkmcnt(0), in front of the first MFMA of a unit: the reads of the next unit
            // follow that MFMA, so seven MFMAs (~110 clocks) stand between them and the wait that covers them
            __builtin_amdgcn_sched_group_barrier(0x100, TM + 2, 0);
#pragma unroll
            for (int u = 0; u < TN; ++u) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (u == 1 || u == 2) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
                else if (u + 1 < TN) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 2 * TM - 1, 0);
            }
        }
    };
    using No = std::integral_constant<bool, false>;
    using Yes = std::integral_constant<bool, true>;
    const int nfull = K / BK, rem = K % BK, nk = nfull + (rem ? 1 : 0);

    // epilogue geometry: a thread owns an 8-column chunk of rows r0, r0 + RPP, ... of each pass
    constexpr int CPR = BN / 8;                                 // chunks per tile row: 28
    constexpr int RPP = NT / CPR;                               // rows per sweep of the workgroup: 18 (504 of 512 threads)
    constexpr int NJ = (HM + RPP - 1) / RPP;                    // rows per thread and pass
    const int cc = tid % CPR, r0 = tid / CPR;
    const bool epi_thread = tid < CPR * RPP;
    // position of 4-float chunk ch of a staged fp32 row: even chunks fill the first half of the row, odd chunks the second (the
    // two chunks of a thread's 8 columns are 28 positions apart: consecutive lanes read consecutive 16-B slots), XOR row & 7
    // inside groups of 8 positions (NCH = 7 x 8: a permutation of the row; the 8 consecutive rows of a ds_write_b128 lane
    // group land on 8 distinct slots of the 128-B write bank row)
    static_assert(NCH % 8 == 0, "XOR inside groups of 8 positions");
    const int wpos = wn * (WTN / 8) + (q >> 1) + (NCH / 2) * (q & 1);          // chunk wn * 28 + 4 tn + q -> position wpos + 2 tn

    int orig = blockIdx.x;
    const uint16_t* src[NPIECE];
    int t = xcd_remap(orig, ntiles);
    int m0 = (t / ntn) * BM, n0 = (t % ntn) * BN;
    sources(src, m0, n0);
    if (0 < nfull) issue(src, 0, 0, No{}); else issue(src, 0, 0, Yes{});

    for (;;) {
#pragma unroll
        for (int a = 0; a < TN; ++a)
#pragma unroll
            for (int b = 0; b < TM; ++b) acc[a][b] = f32x4v{0, 0, 0, 0};

        // ---- main loop: at the top of step s its loads are the only group in flight; wait for them, barrier (the other stage
        //      is then free for everyone — on the first step of a tile that is the previous tile's epilogue LDS), issue step
        //      s + 1 into it, multiply step s.  Raw s_barrier: __syncthreads() would drain vmcnt.
        auto top_of_step = [&](int s) {
            wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (s + 1 < nk) { if (s + 1 < nfull) issue(src, (s + 1) * BK, (s + 1) & 1, No{}); else issue(src, (s + 1) * BK, (s + 1) & 1, Yes{}); }
        };
        for (int s = 0; s < nfull; ++s) {
            top_of_step(s);
            step(s & 1, 8, No{});                               // (every fragment read is consumed by an MFMA of this step)
        }
        if (rem) {
            top_of_step(nfull);
            step(nfull & 1, rem >> 3, Yes{});
        }

        // ---- next tile: its first K-step goes to stage 0 now, behind a barrier (every wave is done with the stages)
        const int n = n0 + cc * 8;
        const bool ncol_ok = n < p.N && epi_thread;             // N % 8 == 0: a chunk is all in or all out
        const int cur_m0 = m0;
        const int next = orig + (int)gridDim.x;
        const bool has_next = next < ntiles;
        __syncthreads();
        if (has_next) {
            orig = next;
            t = xcd_remap(orig, ntiles);
            m0 = (t / ntn) * BM; n0 = (t % ntn) * BN;
            sources(src, m0, n0);
            kb = 0; kin = 0;
            if (0 < nfull) issue(src, 0, 0, No{}); else issue(src, 0, 0, Yes{});
        }

        // ---- epilogue: four passes of 64 rows: accumulators -> LDS (fp32, swizzled [64][224]) -> (row, 8 columns) chunks
        u32x4v braw = u32x4v{0, 0, 0, 0};
        if constexpr (EPI == EPI_BIAS) {
            if (p.bias && ncol_ok) braw = *reinterpret_cast<const u32x4v*>(p.bias + n);
        }
        float bv[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bv[2 * e] = __uint_as_float(braw[e] << 16);
            bv[2 * e + 1] = __uint_as_float(braw[e] & 0xFFFF0000u);
        }
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) {
            if (pass) __syncthreads();                          // the previous pass has been read
            if (wm == pass) {
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                    for (int tm = 0; tm < TM; ++tm) {
                        const int ml = tm * 16 + l15;
                        *reinterpret_cast<f32x4v*>(ctile + ml * BN + (((wpos + 2 * tn) ^ (l15 & 7)) << 2)) = acc[tn][tm];
                    }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int row = r0 + j * RPP, m = cur_m0 + pass * HM + row;
                if (row >= HM || m >= p.M || !ncol_ok) continue;
                const f32x4v lo = *reinterpret_cast<const f32x4v*>(ctile + row * BN + ((cc ^ (row & 7)) << 2));
                const f32x4v hi = *reinterpret_cast<const f32x4v*>(ctile + row * BN + (((cc + NCH / 2) ^ (row & 7)) << 2));
                float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += bv[e];
                st_out16(p.out + (int64_t)m * p.ldo + n,
                         u32x4v{f2bf_pair(v[0], v[1]), f2bf_pair(v[2], v[3]), f2bf_pair(v[4], v[5]), f2bf_pair(v[6], v[7])});
            }
        }
        if (!has_next) break;
        // (the first top_of_step of the next tile starts with a barrier: nobody loads into stage 1 — this epilogue's LDS —
        //  before every thread is past its reads)
    }
}

}  // namespace gemm
}  // namespace cream
