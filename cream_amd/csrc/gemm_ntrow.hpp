// gemm_ntrow.hpp — the full-row NT tile 256 x BN (BN = 384 / 320 = the whole output width) for the backward's input gradients
// (gfx950): fc1 dgrad dc = dh . W1^T, qkv dgrad da = dqkv . Wqkv^T in contraction segments, proj dgrad at E / 64 heads.
//
// Reference semantics: as gemm_mfma.hpp — the input gradients autograd derives for LinearSuper.forward / qkv_super.forward
// (AutoFormer/model/module/Linear_super.py:38-54, qkv_super.py:45-55), computed on the transposed operand copies of the weights.
//     C(M x N) = A(M x K) . B(N x K)^T      N == BN exactly, both operands K-contiguous, bf16, fp32 accumulate, bf16 result
//
// Why its own kernel: in the step these products run beside the weight-gradient stream, which holds half the
// chip.  The 256 x 192 tile needs two workgroups per 256-row panel — 198 workgroups for 99 panels, both of which ingest the same
// 256 x K panel of A on different CUs.  One workgroup per panel ingests 256 + BN rows per K-step where two of them ingest
// 2 x 256 + BN, and the product needs 99 CUs once instead of 198 CU slots in two rounds.
//
//   * 512 threads = 4 (m) x 2 (n) waves, wave tile 64 x BN / 2 = 2 x 6 (BN = 384) or 2 x 5 (BN = 320) blocks of
//     v_mfma_f32_32x32x16_bf16: 192 / 160 accumulator registers, one persistent workgroup per CU walking row panels
//     blockIdx.x, + gridDim.x, ...  Eight waves share four SIMDs, so a wave has HALF a SIMD's 512-entry file: 256 registers for
//     accumulators, fragments and addressing together (__launch_bounds__(512, 1) asks for no more than the one workgroup the
//     LDS allows; it does not widen the file).  Hence the streamed fragments below, and `here()`;
//   * same contraction order per output element as gemm_nt_kernel / gemm_nt8: the chain of an element adds 16 K-elements per
//     MFMA in ascending K (swapped product: a lane owns one output row), so results are bit-identical to the tiles it replaces;
//   * LDS: TWO 64-deep stages of (256 + BN) rows x 128 B = 160 KB at BN = 384 (the CU's whole LDS), 144 KB at BN = 320.  Chosen
//     over three or four 32-deep stages because it keeps the LDS image, the swizzle and the per-K-step barrier count of
//     gemm_nt_kernel, and one K-step of MFMA work per SIMD (2 waves x 48 MFMAs x 32 clocks = 3.1k clocks) already covers the
//     operand latency the two-stage tiles run with.  No stage is spare for the epilogue: it stages through stage 1, which is dead
//     once the last K-step has been multiplied (stage 0 receives the first K-step of the workgroup's next panel meanwhile);
//   * operands go global -> LDS directly (global_load_lds_dwordx4) in 1-KB pieces of 8 rows, piece wave + 8 i of a stage per
//     wave: scalar base (panel origin and K offset: SALU only) plus one 32-bit byte offset per lane and piece — the B offsets
//     never change (n0 = 0), the A offsets change per panel only where the last panel is ragged; no VALU on the request path.
//     The requests are asm statements, so the compiler adds no vmcnt(0) of its own: the waits are counted by hand —
//     vmcnt(0) at the top of a K-step (its loads are the only ones in flight), vmcnt(stores of the epilogue) at the first K-step
//     behind the epilogue of a full panel (the stores are younger than that K-step's loads and drain under it);
//   * LDS image [row][8 chunks of 16 B] with the SOURCE chunk XOR (row >> 1) & 7, as gemm_nt_kernel: a ds_read_b128 of the
//     32x32x16 operand (lane l: row l & 31, chunk (2 ks + (l >> 5)) ^ ((l & 31) >> 1) & 7) serves 16 lanes per pass — 16
//     consecutive rows at one chunk index c: rows 2 j, 2 j + 1 share a 256-B bank row and sit in its two 128-B halves, and the
//     eight row pairs carry the eight values c ^ j: sixteen distinct 16-B slots, no conflict.  The pieces of a wave are 64 rows
//     apart, so one swizzle term serves all of them;
//   * per 16-deep sub-step a wave reads 2 A and 6 (5) B fragments for 12 (10) MFMAs.  The fragments stream: a B fragment is
//     read two units (one unit = its 2 MFMAs, 64 clocks) ahead of its MFMAs, the A fragments of the next sub-step three units
//     before the current one ends (pinned with sched_group_barrier): 28 fragment registers live at the peak, not 64;
//   * the K tail (K % 64 != 0, K % 8 == 0) is ZERO-FILLED: in the last K-step the chunks beyond K are fetched from a 16-byte
//     block of zeros (per-lane addresses, that K-step only), so the loop body has one form and multiplies zeros x zeros;
//   * epilogue without a workgroup barrier, as gemm_nt8: a wave packs its accumulators to bf16, pairs 8-byte runs into 16-byte
//     chunks with v_permlane32_swap and turns 32 x 64 (the odd fifth block of BN = 320: 32 x 32) sub-tiles through ITS OWN 4 KB
//     of stage 1, so that every store is 16 bytes per lane and covers whole 128-byte (64-byte) row runs; stores carry the
//     non-temporal hint (profiles/r05_nt_out_stores.md).  Staging positions are XOR-swizzled with the row (8 consecutive lanes
//     of a ds_write_b128 group hit 8 distinct 16-B slots).
// Addressing: the NtParams contract — kseg / kseg_stride segments of the contraction on B, nseg row segments, lda / ldb / ldo as
// given, rows beyond M never stored (their loads are clamped to row M - 1).
// Limits (the launcher routes elsewhere otherwise): N == BN, K % 8 == 0, 256 lda and the B extent fit 31-bit element offsets.
#pragma once
#include "gemm_mfma.hpp"
#include "gemm_nt8.hpp"

namespace cream {
namespace gemm {

constexpr int NTROW_BM = 256;
__host__ __device__ constexpr int ntrow_lds_bytes(int BN) { return nt_lds_bytes(NTROW_BM, BN, 2); }

// one 1-KB piece: scalar base + 32-bit per-lane byte offset -> LDS at the wave-uniform lds_dst + 16 lane.  M0 is restored.
__device__ __forceinline__ void ntrow_dma(const void* base, uint32_t off, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(off), "s"(lds_dst), "s"(base) : "memory");
}

template <int BN>
__global__ __launch_bounds__(512, 1) void gemm_ntrow_kernel(const NtParams p)
{
    constexpr int BM = NTROW_BM, BK = 64, NW = 8;
    constexpr int WTM = 64, WTN = BN / 2, TM = WTM / 32, TN = WTN / 32;     // wave tile: 2 x 6 / 2 x 5 blocks of 32 x 32
    constexpr uint32_t STAGE_B = (BM + BN) * BK * 2;                        // bytes per stage
    constexpr int NPA = BM / 8 / NW, NPB = BN / 8 / NW;                     // 1-KB pieces per wave and stage: 4 of A, 6 / 5 of B
    constexpr int NCG = (TN + 1) / 2;                                       // epilogue column groups of two blocks (the last may hold one)
    constexpr int NS = TM * (4 * (TN / 2) + 2 * (TN % 2));                  // stores a wave issues in the epilogue of a full panel
    static_assert(BN % 64 == 0 && (BN / 8) % NW == 0 && WTN % 32 == 0, "tile");
    static_assert(NW * 4096 <= STAGE_B && NS <= 63, "epilogue staging inside stage 1; vmcnt immediate");
    char* const smem = LdsBlock<ntrow_lds_bytes(BN)>::get();
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)reinterpret_cast<uintptr_t>(smem));

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 5, c32 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int npanels = (p.M + BM - 1) / BM;
    const int K = p.K, nfull = K / BK, rem = K % BK, nk = nfull + (rem ? 1 : 0);

    // ---- staging: piece wave + 8 i holds stage rows prow + 64 i (A: i < NPA, then B); one k-chunk per lane for all of them
    const int prow = wave * 8 + (lane >> 3);
    const int cch = ((lane & 7) ^ ((prow >> 1) & 7)) * 8;
    uint32_t offA[NPA], offB[NPB];                                          // BYTE offsets from the panel's A origin / from p.B
#pragma unroll
    for (int j = 0; j < NPB; ++j) {
        const int n = prow + 64 * j;                                        // < BN == N
        const int seg = (n >= p.nseg) + (n >= 2 * p.nseg);                  // at most 3 row segments: no division
        offB[j] = (uint32_t)(seg * (int)p.nseg_stride + (n - seg * p.nseg) * (int)p.ldb + cch) * 2u;
    }
    // (a value the compiler must take as new where it stands: the A offsets of a panel, the 64-bit addresses of the tail
    //  K-step and the epilogue's row pointers are loop-invariant, and hoisted out of the K loop they cost more registers than a wave has beside its accumulators)
    auto here = [](uint32_t v) -> uint32_t { asm volatile("" : "+v"(v)); return v; };
    auto lane_now = []() -> int {                                           // the lane id, recomputed where it is needed
        uint32_t l;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
        return (int)l;
    };
    auto set_panel = [&](int m0) {
        const int ln = lane_now(), pr = wave * 8 + (ln >> 3), ch = ((ln & 7) ^ ((pr >> 1) & 7)) * 8;     // = prow, cch
#pragma unroll
        for (int i = 0; i < NPA; ++i) offA[i] = (uint32_t)(min(pr + 64 * i, p.M - 1 - m0) * (int)p.lda + ch) * 2u;
    };
    int64_t kb = 0;                                                         // K offset of the B operand (contraction segments)
    int kin = 0;
    // K-step k0 of the panel at m0 -> stage buf
    auto issue = [&](int m0, int k0, int buf, auto tail) {
        const char* baseA = reinterpret_cast<const char*>(p.A + (int64_t)m0 * p.lda + k0);
        const char* baseB = reinterpret_cast<const char*>(p.B + kb);
        const uint32_t dst = lds0 + (uint32_t)buf * STAGE_B + (uint32_t)wave * 1024u;
        const bool valid = k0 + cch < K;                                    // (tail only) this lane's chunk lies inside K
#pragma unroll
        for (int i = 0; i < NPA; ++i) {
            if constexpr (decltype(tail)::value)
                nt8_dma(valid ? baseA + here(offA[i]) : reinterpret_cast<const char*>(g_nt8_zero), dst + (uint32_t)i * (NW * 1024u));
            else ntrow_dma(baseA, offA[i], dst + (uint32_t)i * (NW * 1024u));
        }
#pragma unroll
        for (int j = 0; j < NPB; ++j) {
            if constexpr (decltype(tail)::value)
                nt8_dma(valid ? baseB + here(offB[j]) : reinterpret_cast<const char*>(g_nt8_zero), dst + (uint32_t)(NPA + j) * (NW * 1024u));
            else ntrow_dma(baseB, offB[j], dst + (uint32_t)(NPA + j) * (NW * 1024u));
        }
        kb += BK;
        kin += BK;
        if (kin >= p.kseg) { kin = 0; kb += p.kseg_stride - p.kseg; }
    };
    using No = std::integral_constant<bool, false>;
    using Yes = std::integral_constant<bool, true>;
    auto issue_step = [&](int m0, int s, int buf) { if (s < nfull) issue(m0, s * BK, buf, No{}); else issue(m0, s * BK, buf, Yes{}); };

    // ---- fragment reads: row c32 of a 32-row block, 16-byte chunk (2 ks + g) ^ sw of its 128-byte row
    const int sw = (c32 >> 1) & 7;
    auto frag = [&](const char* tile, int row, int chunk) -> bf16x8 {
        return *reinterpret_cast<const bf16x8*>(tile + row * (BK * 2) + ((chunk ^ sw) << 4));
    };
    f32x16 acc[TN][TM];
    auto step = [&](int buf) {
        const char* At = smem + (uint32_t)buf * STAGE_B;
        const char* Bt = At + BM * BK * 2;
        // A K-step is NU = 4 TN units of one B fragment and its TM MFMAs (sub-step ks = u / TN, block tn = u % TN).  Eight waves
        // share four SIMDs: a wave has 256 registers, 192 / 160 of them accumulators, so the fragments STREAM — a B fragment is
        // read AHEAD units (AHEAD x TM x 32 clocks) before its MFMAs, the two A fragments of sub-step ks + 1 three units before
        // the end of sub-step ks: 2 x 2 + 3 fragments (28 registers) live at the peak
        constexpr int NU = (BK / 16) * TN, AHEAD = 2;
        bf16x8 fa[2][TM], fb[NU];
        auto ra = [&](int ks) {
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[ks & 1][i] = frag(At, wm * WTM + i * 32 + c32, ks * 2 + g);
        };
        auto rb = [&](int u) { fb[u] = frag(Bt, wn * WTN + (u % TN) * 32 + c32, (u / TN) * 2 + g); };
        // program order = the order the schedule below pins
        ra(0);
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) rb(u);
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if (u + AHEAD < NU) rb(u + AHEAD);
            if (u % TN == TN - 3 && u / TN + 1 < BK / 16) ra(u / TN + 1);
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
                acc[u % TN][tm] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[u], fa[(u / TN) & 1][tm], acc[u % TN][tm], 0, 0, 0);
        }
        // a unit's reads follow its first MFMA: the wait in front of the NEXT unit's first MFMA covers an older read only
        __builtin_amdgcn_sched_group_barrier(0x100, TM + AHEAD, 0);
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int nrd = (u + AHEAD < NU ? 1 : 0) + ((u % TN == TN - 3 && u / TN + 1 < BK / 16) ? TM : 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (nrd == 1) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            else if (nrd == TM) __builtin_amdgcn_sched_group_barrier(0x100, TM, 0);
            else if (nrd == TM + 1) __builtin_amdgcn_sched_group_barrier(0x100, TM + 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, TM - 1, 0);
        }
    };

    // ---- epilogue geometry: this wave's staging tile in stage 1
    char* const stg = smem + STAGE_B + wave * 4096;

    int panel = blockIdx.x, m0 = panel * BM;
    set_panel(m0);
    issue_step(m0, 0, 0);
    bool epi_pending = false;                                               // (wave-uniform) exactly NS stores are younger than the K-step in flight

    for (;;) {
#pragma unroll
        for (int a = 0; a < TN; ++a)
#pragma unroll
            for (int b = 0; b < TM; ++b) acc[a][b] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

        // ---- main loop: at the top of step s its loads are the only group in flight (behind an epilogue: plus that epilogue's
        //      stores, which are younger); wait for them, barrier (the other stage is then free for everyone — on the first step
        //      of a panel that is the previous panel's epilogue staging), issue step s + 1 into it, multiply step s
        for (int s = 0; s < nk; ++s) {
            if (s == 0 && epi_pending) wait_vmcnt<NS>(); else wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (s + 1 < nk) issue_step(m0, s + 1, (s + 1) & 1);
            step(s & 1);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }

        // ---- next panel: its first K-step goes to stage 0 now, behind a barrier (every wave is done with both stages)
        const int cur_m0 = m0;
        const int next = panel + (int)gridDim.x;
        const bool has_next = next < npanels;
        nt_lds_barrier();
        if (has_next) {
            panel = next; m0 = next * BM;
            set_panel(m0);
            kb = 0; kin = 0;
            issue_step(m0, 0, 0);
        }

        // ---- epilogue: per wave, 32-row x 64-column (32-column) sub-tiles through its own 4 KB of stage 1
        const bool full = cur_m0 + BM <= p.M;
        const int el = lane_now(), eg = el >> 5, ec32 = el & 31;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
#pragma unroll
            for (int cg = 0; cg < NCG; ++cg) {
                const int nb = (2 * cg + 2 <= TN) ? 2 : 1;                  // blocks in this group (compile-time after unrolling)
                const int rowb = nb * 64;                                   // bytes per staged row
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    if (b >= nb) continue;
                    const f32x16& av = acc[2 * cg + b][tm];
                    uint32_t pk[8];                                         // pk[2 r4 + h]: columns 8 r4 + 4 g + 2 h, + 1 of the block
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
                        for (int h = 0; h < 2; ++h) pk[2 * r4 + h] = f2bf_pair(av[4 * r4 + 2 * h], av[4 * r4 + 2 * h + 1]);
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        // 8-byte runs of r4 = 2 j and 2 j + 1: after the half exchange lanes 0-31 hold columns 16 j .. + 7, lanes
                        // 32-63 columns 16 j + 8 .. + 15 of the block (cdna_hip_programming.md T21)
                        auto r0 = __builtin_amdgcn_permlane32_swap(pk[4 * j], pk[4 * j + 2], false, false);
                        auto r1 = __builtin_amdgcn_permlane32_swap(pk[4 * j + 1], pk[4 * j + 3], false, false);
                        const int chunk = b * 4 + 2 * j + eg;
                        const int pos = nb == 2 ? (chunk ^ (ec32 & 7)) : (chunk ^ ((ec32 >> 1) & 3));
                        *reinterpret_cast<u32x4v*>(stg + ec32 * rowb + (pos << 4)) = u32x4v{r0[0], r1[0], r0[1], r1[1]};
                    }
                }
                // after the turn: 8 (4) lanes per row, 8 (16) rows per store instruction
                const int cpr = nb * 4, rps = 64 / cpr;                     // chunks per row, rows per store
                const int rrow = el / cpr, rlc = el % cpr;
                const int ncol = wn * WTN + cg * 64 + rlc * 8;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i * rps >= 32) continue;
                    const int rr = rrow + rps * i, m = cur_m0 + wm * WTM + tm * 32 + rr;
                    const int pos = nb == 2 ? (rlc ^ (rr & 7)) : (rlc ^ ((rr >> 1) & 3));
                    const u32x4v v = *reinterpret_cast<const u32x4v*>(stg + rr * rowb + (pos << 4));
                    if (full || m < p.M) st_out16(p.out + (int64_t)m * p.ldo + ncol, v);
                }
            }
        }
        if (!has_next) break;
        epi_pending = full;
        // (the first K-step of the next panel starts with a barrier: nobody loads into stage 1 — this epilogue's staging —
        //  before every wave is past its reads)
    }
}

}  // namespace gemm
}  // namespace cream
