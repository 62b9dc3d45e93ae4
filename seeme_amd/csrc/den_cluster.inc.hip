// den_cluster.inc.hip -- the sampling loop with ONE SAMPLE SPLIT OVER C WORKGROUPS (CUs)  (included by den_kernels.hip).
//
// Reference: the same chain as k_den_sample -- MldDenoiser.forward (mld_denoiser.py:151-244) with
// LinearTemporalDiffusionTransformerDecoderLayer (mdiff_transformer.py:286-304) inside SkipTransformerEncoder
// (cross_attention.py:67-83), driven by MLD._diffusion_reverse (mld.py:467-497).
//
// Why: at B = 32 (BASELINE configs[1]) k_den_sample keeps 32 of 256 CUs busy and each of them is bound by the 118 GB/s of
// one CU's vector-memory path (84 us per step for the 9 MB image).  Here a "cluster" of C = 2, 4 or 8 workgroups (one per CU)
// owns a sample: the three big matrices of a layer are split between them, the small ones are replicated, and a step needs
// TWO exchanges per layer:
//
//   A   in_proj' (q | k | W_o v [| y = skip linear, folded: layers 3, 4])  COLUMN-split by dims: CU c computes dims
//       c S .. c S + S - 1 (S = 256 / C) of q, k, v' (and y) from the full input vector (replicated)
//   X1  every CU publishes v'[S] (, y[S]) and its partial scores q.k over its dims (self, condition, time token); every CU
//       gathers them -> softmax over the 2 + N tokens, attention output, + residual, norm1: replicated, bit-identical
//   B   linear1 COLUMN-split (1024 / C hidden units per CU), ReLU                      -- no exchange
//   C   linear2 ROW-split over the CU's hidden units -> 256 partial sums per CU
//   X2  all-reduce of the 256 partial sums (fixed order of addition) -> + bias, residual, norm2, + ca_block term: replicated
//   D E F  ffn.linear1 / linear2 / proj_out (64 + 64 + 128 KB at 16 bit) REPLICATED on every CU -- no exchange
//
// The skip linears of layers 3 and 4 are folded into that layer's in_proj' on the host ([W_in' W_s ; W_s] acting on
// cat[x, skip], seeme_amd/mld_denoiser.py): no extra exchange.  One attention head, one condition token (the ca_block term
// comes from seeme_denoiser_ca_tables), no CFG: the configuration BASELINE's headline names; everything else stays on
// k_den_sample.
//
// Exchange = cdna_hip_programming.md Guideline 16, R2: every value travels as one aligned 8-byte {tag = epoch, value}
// granule written by ONE store; the epilogue wave of every CU re-reads its granules with sc1 loads (bypass L1) until every
// tag equals the epoch.  The epoch counts exchanges within the launch (never 0); the host zeroes the granule buffer before
// every launch.  X1 and X2 alternate, so a buffer is only rewritten after every reader has passed the exchange in between.
// Stores are write-through (sc1: visible to any CU of the chip) unless the cluster has established in its first exchange
// (which is always write-through) that all its workgroups report the same XCC id: then plain stores, which stay in that
// XCD's L2 where the peers' sc1 loads find them (probes/xchg_test.hip: 1.25 us instead of 2.0 us per exchange at C = 8).
// Correctness never depends on placement; speed does (blockIdx b and b + 8 share an XCD under round-robin dispatch).
// Every spin is bounded: a cluster that gives up sets a word of the exchange buffer's header and finishes without waiting.
//
// Weights: `units` of 8 waves x UL wave-loads x 1 KiB in order of use ([layer][CU][unit][wave][load][lane][16 B]); a wave-load
// is the MFMA B operand of one (16-output tile, k-block) pair.  A ring of RU units in registers runs RU units (half a layer)
// ahead of the consumer, across stage, layer and step boundaries.
//
// Who consumes a unit: all eight waves, each its eighth (fp32 images, C = 2 and 4, two condition tokens, k_den_cluster_ms) -- or, for the
// 16-bit images at C = 8 with one condition token (the B <= 32 default), two groups of four waves that take the six GEMV phases in turn, so
// that the group without a phase requests weights while the other computes (ClGrp below).  Same image, same sums, bit for bit.

#define DCL_MAGIC_EPOCH 0x7fffffffu
#define DCL_SPIN_LIMIT (1u << 22)

typedef __attribute__((address_space(1))) unsigned long long dcl_gu64;

template <typename WT> struct ClW {
    static constexpr int KL = WT::MFMA ? 32 : 16;      // k per wave-load (16-bit: v_mfma_f32_16x16x32; fp32: 4 x v_mfma_f32_16x16x4)
    static constexpr int UL = 256 / KL;                // wave-loads per unit
    static constexpr int RU = WT::MFMA ? 4 : 2;        // units in the register ring (32 x 16 B per lane either way)
    static constexpr unsigned UNIT_BYTES = 8u * UL * 1024u;
};
template <int C, bool Q = false> struct ClG {          // Q: several condition tokens -- the ca_block keeps its query and proj_out stages (G, H)
    static constexpr int S = 256 / C;                  // dims of q / k / v' / y per CU
    static constexpr int NB = 1024 / C;                // hidden units of the sa_block MLP per CU
    static constexpr int TA = S / 32;                  // tiles per wave in stage A (waves 0,1: q; 2,3: k; 4,5: v'; 6,7: y) = units per k-half
    static constexpr int TB = 8 / C;                   // tiles per wave in stage B = units of stage B = units of stage C
    static constexpr int U_A = 0, U_AS = TA, U_B = 2 * TA, U_C = U_B + TB;
    static constexpr int U_G = U_C + TB, U_H = U_G + 1;                       // (Q only) ca query: one unit, waves < S / 16; ca proj_out: two units
    static constexpr int U_D = Q ? U_H + 2 : U_C + TB, U_E = U_D + 1, U_F = U_E + 1, NU_REAL = U_F + 2;
    static constexpr int NU = (NU_REAL + 3) / 4 * 4;   // padded with phantom units: ring positions repeat per layer
    static constexpr int SC = Q ? 8 : 4;               // partial-score granules a CU publishes (2 + N values, padded)
    static constexpr int X1_G = 2 * S + SC;            // granules a CU publishes in X1: v'[S] | y[S] | partial scores [SC]
    // granules per sample: boot [16] | X1 [C][X1_G] | X2 [C][256] | X3 [C][8] (Q: partial softmax / key products of the ca query)
    static constexpr int G_BOOT = 0, G_X1 = 16, G_X2 = G_X1 + C * X1_G, G_X3 = G_X2 + C * 256, G_TOTAL = G_X3 + (Q ? C * 8 : 0);
    static constexpr int EPL = Q ? 3 : 2;              // exchanges (epochs) per layer
};
#define DCL_HDR_BYTES 256   // header of the exchange buffer: [0] give-up code, [1] clusters that used L2-local stores

template <typename WT> struct ClRing { u32x4 r[ClW<WT>::RU][ClW<WT>::UL]; };

struct ClArgs {
    const void* wgc; unsigned wgc_bytes; const float* vp;
    DenLayout lay;
    SeemeSampleArgs s;
    unsigned long long* xg;      // granules (behind the header)
    unsigned* hdr;
    int placement, flags, clusters;
    int spc;                     // k_den_cluster_ms: samples per cluster (<= 8)
};

// ---- one unit of the weight stream -> its ring slot
template <typename WT, int C, bool Q, int U>
__device__ __forceinline__ void cl_issue(ClRing<WT>& ring, int wave, unsigned voff, __amdgpu_buffer_rsrc_t rsrc,
                                         unsigned base_cur, unsigned base_next, bool skip_cur, bool skip_next) {
    typedef ClW<WT> W; typedef ClG<C, Q> G;
    constexpr int UU = U % G::NU;
    constexpr bool NXT = U >= G::NU;
    static_assert(U < 2 * G::NU && G::NU % W::RU == 0, "ring positions must repeat per layer");
    if constexpr (UU >= G::NU_REAL) return;            // phantom unit (padding of the layer program)
    if constexpr (Q && UU == G::U_G) { if (wave >= G::S / 16) return; }       // the ca query has S / 16 tiles: one per wave
    const bool sk = NXT ? skip_next : skip_cur;
    if constexpr (UU < G::U_B) {                       // stage A: the skip half only where the layer has a skip linear; the y waves likewise
        if constexpr (UU >= G::U_AS) { if (!sk) return; }
        if (wave >= 6 && !sk) return;
    }
    const unsigned soff = (NXT ? base_next : base_cur) + (unsigned)UU * W::UNIT_BYTES;
#pragma unroll
    for (int i = 0; i < W::UL; ++i) ring.r[UU % W::RU][i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff + (unsigned)(i * 1024), 0);
}

// ---- GEMV input vectors in LDS.  16-bit weights: MFMA A-operand fragments [k-block][k-group 4][row 4][8 halves], row p =
// part p of the fp32 value (put_x); fp32 weights: the plain fp32 vector.
struct ClX { const char* base; int foff; int kbs; };     // kbs: bytes per k-block of the fragment buffer (rows x 4 k-groups x 16 B)
template <typename WT>
__device__ __forceinline__ ClX cl_xin(const float* buf, int lane) {
    ClX x; x.base = reinterpret_cast<const char*>(buf);
    x.foff = WT::MFMA ? ((lane >> 4) * 4 + ((lane & 15) & 3)) * 16 : (lane >> 4) * 16;
    x.kbs = WT::MFMA ? 256 : 64;
    return x;
}
template <typename WT>
__device__ __forceinline__ void cl_put1(float* buf, int k, float v) {     // one element (an MFMA output lane)
    if constexpr (!WT::MFMA) { buf[k] = v; }
    else {
        char* dst = reinterpret_cast<char*>(buf) + (((k >> 5) * 4 + ((k >> 3) & 3)) * 4) * 16 + (k & 7) * 2;
        if constexpr (WT::HALF) {
            const _Float16 hi = (_Float16)v;
            *reinterpret_cast<_Float16*>(dst) = hi;
            *reinterpret_cast<_Float16*>(dst + 16) = (_Float16)((v - (float)hi) * DEN_F16_LO_SCALE);
        } else {
            const __bf16 hi = (__bf16)v; const float r1 = v - (float)hi; const __bf16 mid = (__bf16)r1;
            *reinterpret_cast<__bf16*>(dst) = hi;
            *reinterpret_cast<__bf16*>(dst + 16) = mid;
            *reinterpret_cast<__bf16*>(dst + 32) = (__bf16)(r1 - (float)mid);
        }
    }
}
// value of the lane's output column from an accumulator (every 16-lane group holds the same 16 columns)
template <typename WT>
__device__ __forceinline__ float cl_out(const f32x4& a) {
    if constexpr (!WT::MFMA) return a.x;
    else if constexpr (WT::HALF) return fmaf(a.y, 1.f / DEN_F16_LO_SCALE, a.x);
    else return a.x + (a.y + a.z);
}

// ---- consume one unit: load i of the unit is load J0 + i of the stage; stage load j = (k-block j / TPW, tile j % TPW)
template <typename WT, int TPW, int J0, int KBOFF>
__device__ __forceinline__ void cl_consume(const u32x4 (&slot)[ClW<WT>::UL], const ClX& x, f32x4 (&acc)[TPW]) {
    typedef ClW<WT> W;
    uint4 a4 = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int i = 0; i < W::UL; ++i) {
        constexpr int dummy = 0; (void)dummy;
        const int j = J0 + i, kb = j / TPW - KBOFF, t = j % TPW;
        if constexpr (WT::MFMA) {
            if (i == 0 || t == 0) a4 = *reinterpret_cast<const uint4*>(x.base + x.foff + kb * x.kbs);
            if constexpr (WT::HALF) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, a4), __builtin_bit_cast(h16x8, slot[i]), acc[t], 0, 0, 0);
            else acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a4), __builtin_bit_cast(bf16x8, slot[i]), acc[t], 0, 0, 0);
        } else {
            if (i == 0 || t == 0) a4 = *reinterpret_cast<const uint4*>(x.base + x.foff + kb * x.kbs);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a4.x), __uint_as_float(slot[i].x), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a4.y), __uint_as_float(slot[i].y), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a4.z), __uint_as_float(slot[i].z), acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a4.w), __uint_as_float(slot[i].w), acc[t], 0, 0, 0);
        }
    }
}
template <int TPW>
__device__ __forceinline__ void cl_pin(f32x4 (&acc)[TPW]) {   // program-order pin (see Acc::pin)
#pragma unroll
    for (int t = 0; t < TPW; ++t) asm volatile("" : "+v"(acc[t]) :: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
template <int TPW>
__device__ __forceinline__ void cl_zero(f32x4 (&acc)[TPW]) {
#pragma unroll
    for (int t = 0; t < TPW; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
}
// NUN consecutive units of one stage from unit U0 on: consume, then re-fill the freed slot with unit U + RU -- inline for the
// first NINL units of the call only.  Stages that end in an exchange (A, C) leave the re-fills of their LAST (up to RU) units
// to cl_refills, after the exchange: loads queued in this CU's vector-memory path right before the publish / poll are latency
// on the exchange (the hand-off's price sits in the consumer CU's own memory queue, MI355X_MICROARCH.md handoff-1to1).  Units
// further than RU from the end of such a stage must re-fill inline: their targets are consumed inside the same stage.
template <typename WT, int C, bool Q, int U0, int NUN, int TPW, int UI0, int KBOFF, int NINL, int... Is>
__device__ __forceinline__ void cl_units(ClRing<WT>& ring, const ClX& x, f32x4 (&acc)[TPW], bool active, int wave, unsigned voff,
                                         __amdgpu_buffer_rsrc_t rsrc, unsigned bc, unsigned bn, bool sc, bool sn, std::integer_sequence<int, Is...>) {
    typedef ClW<WT> W;
    (([&] {
        constexpr int U = U0 + Is;
        if (active) { cl_consume<WT, TPW, (UI0 + Is) * W::UL, KBOFF>(ring.r[U % W::RU], x, acc); }
        cl_pin<TPW>(acc);
        if constexpr (Is < NINL) {
            cl_issue<WT, C, Q, U + W::RU>(ring, wave, voff, rsrc, bc, bn, sc, sn);
            cl_pin<TPW>(acc);
        }
    }()), ...);
}
template <typename WT, int C, bool Q, int U0, int... Is>
__device__ __forceinline__ void cl_refills(ClRing<WT>& ring, int wave, unsigned voff, __amdgpu_buffer_rsrc_t rsrc, unsigned bc, unsigned bn,
                                           bool sc, bool sn, std::integer_sequence<int, Is...>) {
    (cl_issue<WT, C, Q, U0 + Is + ClW<WT>::RU>(ring, wave, voff, rsrc, bc, bn, sc, sn), ...);
    __builtin_amdgcn_sched_barrier(0);
}
constexpr int cl_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- the windowed load schedule (every wave consumes every unit: k_den_cluster with two condition tokens or C = 4, and k_den_cluster_ms; the
// 16-bit images at C = 8 with one condition token keep the windows and their flags but fill them by wave group, ClGrp below).  Issuing a 1-KiB wave-load costs the CU's address path 16 cycles
// and the issuing wave waits its turn, so re-fills requested inline are exposed time: at a phase start every wave stands in the queue (phase B:
// 2.4 k of its 4 k cycles), before a publish the stores stand behind them.  But while the epilogue wave is in an exchange or in its serial
// vector algebra the other seven waves have nothing to do.  So they request ONE unit in each such window (56 KiB = 900 cycles of the path):
//   W?A  right after the epilogue wave has PUBLISHED (its stores go first), while it sleeps DCL_POLL_SLEEP x 64 cycles before its first poll:
//        the peers' granules are not due earlier than that, and the poll then finds the queue drained instead of standing behind the unit;
//   W?B  after its sweep, during the vector algebra;   W3  during the ffn epilogue
// -- released through words in LDS, accessed through the LDS address space (through a generic pointer the compiler emits flat loads waited for
// with vmcnt(0): seven waves spinning on those sit in the very queue the polls need).  The epilogue wave requests its eighth of a window's
// unit BEFORE it releases the others (behind them it would wait out their backlog).  The rest (the next layer's A0, A1) goes out after phase F.
//   units A0 A1 | B | C | D | E | F0 F1 = 0..7:  W1A B C | W1B D | W2A E | W2B F0 | W3 F1 | after F: next A0 A1
#ifndef DCL_POLL_SLEEP
#define DCL_POLL_SLEEP 12
#endif
template <int... Us> using ClSeq = std::integer_sequence<int, Us...>;
template <int C, bool MF, bool Q> struct ClSched { static constexpr bool WIN = false; static constexpr int PRO = 0; typedef ClSeq<> W1A, W1B, W2A, W2B, WXA, WXB, W3, AF; };
// "Just in time": a unit goes out in the window before the phase that consumes it; only the next layer's A is requested inline (after F).
// (The <8, true, false> table is k_den_cluster_ms's at C = 8 since k_den_cluster runs that case on two wave groups.)
// PRO: units in flight at a layer's start.  (Measured against it and dropped: "early", every unit one window ahead of the inline scheme, with
// the next layer's B and C still inline in phase F; and just in time with two units in the second exchange window as well.)
template <> struct ClSched<8, true, false> { static constexpr bool WIN = true; static constexpr int PRO = 2; typedef ClSeq<> WXA, WXB; typedef ClSeq<2, 3> W1A; typedef ClSeq<4> W1B; typedef ClSeq<5> W2A; typedef ClSeq<6> W2B;
                                             typedef ClSeq<7> W3; typedef ClSeq<8, 9> AF; };
// Two condition tokens (Q: the ca_block keeps its query G and proj_out H stages and a third exchange X3), just in time as well:
//   units A 0 | AS 1 | B 2 | C 3 | G 4 | H 5 6 | D 7 | E 8 | F 9 10 | (11 phantom);  ring slot = U % 4
//   W1A B C | W1B G | W2A H0 | W2B H1 | WXA (X3 published) D | WXB (X3 swept) E | W3 (ffn epilogue) F0 F1 | after F: next A, AS
template <> struct ClSched<8, true, true> { static constexpr bool WIN = true; static constexpr int PRO = 2; typedef ClSeq<2, 3> W1A; typedef ClSeq<4> W1B; typedef ClSeq<5> W2A; typedef ClSeq<6> W2B;
                                            typedef ClSeq<7> WXA; typedef ClSeq<8> WXB; typedef ClSeq<9, 10> W3; typedef ClSeq<12, 13> AF; };
// Four CUs per sample (16-bit images, 32 < B <= 64): units A 0 1 | AS 2 3 | B 4 5 | C 6 7 | D 8 | E 9 | F 10 11;
// with two condition tokens: ... | G 8 | H 9 10 | D 11 | E 12 | F 13 14 | (15 phantom).  k_den_cluster_ms runs the same tables.
template <> struct ClSched<4, true, false> { static constexpr bool WIN = true; static constexpr int PRO = 4; typedef ClSeq<4, 5> W1A; typedef ClSeq<6, 7> W1B; typedef ClSeq<8, 9> W2A; typedef ClSeq<10, 11> W2B;
                                             typedef ClSeq<> WXA, WXB; typedef ClSeq<12, 13> W3; typedef ClSeq<14, 15> AF; };
template <> struct ClSched<4, true, true> { static constexpr bool WIN = true; static constexpr int PRO = 4; typedef ClSeq<4, 5> W1A; typedef ClSeq<6, 7> W1B; typedef ClSeq<8, 9> W2A; typedef ClSeq<10> W2B;
                                            typedef ClSeq<11> WXA; typedef ClSeq<12> WXB; typedef ClSeq<13, 14> W3; typedef ClSeq<16, 17, 18, 19> AF; };
template <typename WT, int C, bool Q, int... Us>
__device__ __forceinline__ void cl_issue_seq(ClRing<WT>& ring, int wave, unsigned voff, __amdgpu_buffer_rsrc_t rsrc, unsigned bc, unsigned bn,
                                             bool sc, bool sn, ClSeq<Us...>) {
    (cl_issue<WT, C, Q, Us>(ring, wave, voff, rsrc, bc, bn, sc, sn), ...);
    __builtin_amdgcn_sched_barrier(0);
}
typedef __attribute__((address_space(3))) volatile int cl_lds_flag;
__device__ __forceinline__ void cl_flag_set(int* f, unsigned v) { *(cl_lds_flag*)f = (int)v; }
__device__ __forceinline__ void cl_flag_wait(const int* f, unsigned v) {      // (set by this workgroup's epilogue wave: always arrives)
    while (*(const cl_lds_flag*)f != (int)v) __builtin_amdgcn_s_sleep(1);
}

// ---- two wave groups (16-bit images, C = 8, one condition token).  A GEMV phase needs four waves, one per SIMD: waves 0 .. 3 (G0, with the
// epilogue wave) run A, C, E, waves 4 .. 7 (G1) run B, D, F.  The group without a phase is free to request weights while the vector-memory
// path is otherwise idle, and its turn in the CU's in-order queue costs the chain nothing.  The image is unchanged: wave w of the group that owns
// a phase plays the stored waves w % 4 and w % 4 + 4 of the unit -- their 2 x 8 wave-loads with the voff of each, their tiles, per tile the
// k-blocks in cl_consume's order -- so every sum is the one the eight-wave schedule formed.  Ring: 2 slots x 16 wave-loads per wave.
//   G0  slot 0: A0 -> C -> next A0      slot 1: A1 -> E -> next A1          G1  slot 0: B -> F0      slot 1: D -> F1
//   X1 published: B (G1) | X1 first poll issued: E, half (G0) | X1 swept: C (G0) | phase B: E, half (G0) | X2 published: D (G1) |
//   X2 swept: F0 (G1) | phase D: next A0 (G0) |
//   phase E + ffn epilogue: F1 in halves (G1) | phase F: next A1 (G0; the skip half, wanted in skip layers only)
// Nothing is requested ahead of a publish (phases A and C end in granule stores), every slot is requested only after its unit was consumed,
// and but for B and A1 -- their slots hold F0 / E until late, and phase A may not request -- every unit is at least a phase ahead.
// The barrier that ends a phase waits for the requesting group too: 64 wave-loads are 1 k cycles of the address path, and the 16 MFMAs of B, D
// or E take 0.55 - 0.6 k: a whole unit per phase makes D last as long as the request (1.0 k), as it made B (0.9 k); half a unit is hidden.
// The other half of E travels behind the FIRST poll of X1 (FPI below): between a publish and the end of its sweep the epilogue wave requests
// that half unit and nothing else, so its first poll stands behind no load, a repeated one behind 32 wave-loads.  (The same for the next A0
// behind X2's first poll was built and measured: 0.008 ms of the pass on top of this, 1.1 - 1.25 x the run-to-run spread, taken out again.)
// DCL_POLL_SLEEP matters since then -- measured at B = 32, and at 12 also at B = 8: at 10 and below the first poll stands in G1's unit B and
// the pass loses what it gained and more, 12 .. 16 measure the same, at 20 the gain is gone.  Stamps: profiles/cluster_wave_groups.txt,
// profiles/cluster_poll_windows.txt.
template <typename WT, int C, bool Q> struct ClGrp { static constexpr bool ON = C == 8 && WT::MFMA && !Q; };
struct ClSchedGrp { static constexpr bool WIN = true; static constexpr int PRO = 0; typedef ClSeq<> W1A, W1B, W2A, W2B, WXA, WXB, W3, AF; };   // (the windows and their flags stay; what goes out in them is listed above)
struct ClRing2 { u32x4 r[2][2][8]; };              // [slot][stored wave w % 4 | w % 4 + 4][wave-load]
// unit at byte offset soff -> slot SLOT; voff: of stored wave w % 4.  on[h] false: stored wave h's loads are not wanted (stage A: the skip half and the y
// waves only where the layer has a skip linear).  They are then requested past the end of the image -- the buffer's range check answers with zeros and
// reads no memory -- instead of branched around: a slot written on one path only is kept twice and copied at the join, and the wait counts of every
// unit requested before it are then those of the path WITH the loads behind them, i.e. vmcnt(0).  H: which of the two stored waves this call requests.
#define DCLG_NOWHERE 0x7fff0000u
template <int SLOT, int H = 3>
__device__ __forceinline__ void clg_issue(ClRing2& ring, unsigned voff, __amdgpu_buffer_rsrc_t rsrc, unsigned soff, bool on0, bool on1) {
    if constexpr (H & 1) {
        const unsigned v0 = on0 ? voff : DCLG_NOWHERE;
#pragma unroll
        for (int i = 0; i < 8; ++i) ring.r[SLOT][0][i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v0, soff + (unsigned)(i * 1024), 0);
    }
    if constexpr (H & 2) {
        const unsigned v1 = on1 ? voff + 4u * 8u * 1024u : DCLG_NOWHERE;
#pragma unroll
        for (int i = 0; i < 8; ++i) ring.r[SLOT][1][i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, v1, soff + (unsigned)(i * 1024), 0);
    }
    __builtin_amdgcn_sched_barrier(0);
}
// consume a slot: cl_consume's stage loads (k-block j / TPW, tile j % TPW) for both stored waves, alternating -- two independent accumulator
// chains per tile index, one fragment read for both; per tile the k-blocks in cl_consume's order
//
// The A-operand fragments of a phase are read AHEAD of its first MFMA (clg_frags: NK k-blocks, back to back), not one k-block at a time in
// front of the MFMAs that use it: only four waves compute in a phase, one per SIMD, so nothing hides an LDS round trip (>= 64 cycles against
// 2 x 16 of the two MFMAs it feeds) -- phase time followed the number of such trips (D: 8 trips 0.96 k cycles, E: 4 trips 0.57 k, the same 16
// MFMAs).  LDS returns in order, so the MFMAs of k-block i wait with lgkmcnt(reads behind it), not lgkmcnt(0).
template <int NK>
__device__ __forceinline__ void clg_frags(uint4 (&f)[NK], const ClX& x) {
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        f[k] = *reinterpret_cast<const uint4*>(x.base + x.foff + k * x.kbs);
        if (k == 0) __builtin_amdgcn_sched_barrier(0);        // (k-block 0 first: left to itself the scheduler requests it last in three of six phases)
    }
}
template <typename WT, int TPW, int NK, int K0>      // f[K0 ..]: the 8 / TPW k-blocks of this unit
__device__ __forceinline__ void clg_consume(const u32x4 (&slot)[2][8], const uint4 (&f)[NK], f32x4 (&acc)[2][TPW]) {
    static_assert(WT::MFMA, "16-bit images only");
    static_assert(K0 + 8 / TPW <= NK, "fragments of the unit");
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = K0 + i / TPW, t = i % TPW;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if constexpr (WT::HALF) acc[h][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, f[k]), __builtin_bit_cast(h16x8, slot[h][i]), acc[h][t], 0, 0, 0);
            else acc[h][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, f[k]), __builtin_bit_cast(bf16x8, slot[h][i]), acc[h][t], 0, 0, 0);
        }
    }
}
// phase A's first k-half (one tile per stored wave): behind the MFMAs of k-block i its fragment register takes k-block i of the NEXT input
// vector (the skip input), so that the second k-half finds its fragments read as well -- sixteen fragments at once do not fit the registers
template <typename WT>
__device__ __forceinline__ void clg_consume_refill(const u32x4 (&slot)[2][8], uint4 (&f)[8], const ClX& xn, f32x4 (&acc)[2][1]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if constexpr (WT::HALF) acc[h][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, f[i]), __builtin_bit_cast(h16x8, slot[h][i]), acc[h][0], 0, 0, 0);
            else acc[h][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, f[i]), __builtin_bit_cast(bf16x8, slot[h][i]), acc[h][0], 0, 0, 0);
        }
        f[i] = *reinterpret_cast<const uint4*>(xn.base + xn.foff + i * xn.kbs);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// value of the lane's tile: 16-lane group g of a wave writes tile g of acc[stored wave][tile]
template <typename WT, int TPW>
__device__ __forceinline__ float clg_out(const f32x4 (&acc)[2][TPW], int lane) {
    const int h = TPW == 2 ? lane >> 5 : lane >> 4, t = TPW == 2 ? (lane >> 4) & 1 : 0;
    float v = cl_out<WT>(acc[0][0]);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int tt = 0; tt < TPW; ++tt) v = (h == hh && t == tt) ? cl_out<WT>(acc[hh][tt]) : v;
    return v;
}

// ---- granules
__device__ __forceinline__ void cl_store_granule(unsigned long long* g, unsigned epoch, float v, bool local) {
    const unsigned long long x = ((unsigned long long)epoch << 32) | __float_as_uint(v);
    if (local) *(volatile dcl_gu64*)g = x;                                                       // stays in this XCD's L2
    else __hip_atomic_store((dcl_gu64*)g, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);         // sc1: write-through
}
__device__ __forceinline__ unsigned cl_tags_ok(const u32x4& a, unsigned epoch) { return (unsigned)(a.y == epoch) & (unsigned)(a.w == epoch); }   // (no short-circuit branches)

// ---- small operands of a layer (everything that is not a matrix).  What THIS CU reads of them falls in two classes:
//   launch-constant  its slices of the skip / in_proj / linear1 biases, the ten LayerNorm and bias vectors of the replicated stages, the sa
//                    K | V' of the sample's condition token: 3 200 floats per layer at C = 8 (3 456 at C = 4, 3 968 at C = 2)
//   changing         the time token's K | V', the ffn AdaLN scale | shift, the tabulated ca term: five rows of 256 floats, selected by the
//                    table row (step, or sample with per-sample timesteps) and the layer
// One condition token (!Q): the constant class of ALL five layers is RESIDENT in LDS (ClRes: 64 KB at C = 8), loaded once in the prologue by
// LDS-DMA; only the five changing rows travel per layer, into the other half of a 2 x 5 KiB double buffer (ClRow).  They are requested by
// waves 1 .. 5 as the OLDEST loads of the X1 window -- before the wave's share of the window's units -- and stored behind those units, in
// front of the barrier that closes the window (where these waves wait out the epilogue wave's sweep and vector algebra anyway): vmcnt
// retires in order, so the store's wait is vmcnt(wave-loads requested behind the row) -- 24 at C = 8: every unit stays in flight -- and
// the row has had the whole exchange to land.  Phases B .. F request and stage nothing.  (Stored at the END of phase B instead, the row
// lives across the join of the epilogue wave's and the other waves' paths: the compiler then copies it at the end of the window, with the
// same vmcnt(24), and counts the first MFMA of B as vmcnt(2) instead of vmcnt(23) -- tried, ISA read, dropped.)
//   (Before: all 22 pieces of the next layer were re-fetched in every layer of every step, one piece per wave at the top of each of B, D
//   and F, stored at the phase's end.  The piece was then the NEWEST load of its wave, so the store drained the whole in-order queue --
//   `s_waitcnt vmcnt(0)` in front of the ds_write of B and D, and at the last MFMA of F -- i.e. the units the windows had requested for
//   LATER phases: three times per layer the ring that is meant to run ahead was emptied inside a phase of a few hundred cycles of work.)
// Residency is per launch and in LDS only: nothing survives the kernel, so no weight, condition or scheduler change can be seen stale.
// Two condition tokens (Q): ~6 000 constant floats per layer do not fit five-fold; ClStage keeps the per-layer staging through registers
// (26 + NL1 + 4 N pieces of at most 1 KiB, one per wave at the top of each of B, C, H, D, F into the other half of a full-layout double buffer).
template <int C> struct ClRes {                        // compact layout of one layer's launch-constant operands (floats)
    static constexpr int S = ClG<C>::S, NB = ClG<C>::NB;
    static constexpr int SKIP_B = 0, IN_B = S;         // [S] skip_b slice | [3][S] q, k, v' slices of in_b
    static constexpr int L1B = 4 * S;                  // [NB] linear1 bias slice
    static constexpr int V5 = L1B + NB;                // n1w n1b l2b n2w n2b   (256 each)
    static constexpr int F1B = V5 + 5 * 256;           // [FF_D]
    static constexpr int V4 = F1B + FF_D;              // f2b fsnw fsnb fo_b    (256 each)
    static constexpr int CT = V4 + 4 * 256;            // sa K | V' of the sample's condition token
    static constexpr int LAYER = CT + 512;
    static constexpr int NL1 = NB > 256 ? NB / 256 : 1;
    static constexpr int NP = 16 + NL1;                // pieces (<= 1 KiB) per layer
    static constexpr int ROWS = 5 * 256;               // one half of the double buffer: time K | time V' | ffn scale | ffn shift | ca term
    static constexpr int FLOATS = SEEME_DEN_NL * LAYER + 2 * ROWS;
};
// prologue: every layer's launch-constant operands -> the resident block, layer 0's changing rows -> half 0 of the double buffer; LDS-DMA,
// the pieces dealt over the eight waves (the caller waits vmcnt(0) and synchronises)
template <int C>
__device__ __forceinline__ void cl_load_resident(int wave, int lane, float* __restrict__ res, const float* __restrict__ vpg, const DenLayout* __restrict__ lay,
                                                 const float* __restrict__ tt_row, const SeemeSampleArgs& A, int b, int c, int ca_R) {
    typedef ClRes<C> R;
    const uint32_t base = lds_addr_of(res);
#pragma unroll 1
    for (int p = wave; p < SEEME_DEN_NL * R::NP + 5; p += DEN_THREADS / 64) {
        const float* src; int d, n = 64;
        if (p >= SEEME_DEN_NL * R::NP) {               // layer 0's changing rows (ca row of a shared timestep table: step 0)
            const int j = p - SEEME_DEN_NL * R::NP;
            d = SEEME_DEN_NL * R::LAYER + j * 256;
            src = j < 2 ? tt_row + j * 256 : (j < 4 ? tt_row + 2560 + 512 + (j - 2) * 256 : A.catab + (size_t)b * ca_R * SEEME_DEN_NL * 256);
        } else {
            const int l = p / R::NP, i = p - l * R::NP;
            const DenLayerOff* __restrict__ L = &lay->L[l];
            const float* vb = vpg + L->skip_b;
            if (i == 0) { src = vb + c * R::S; d = R::SKIP_B; n = R::S / 4; }
            else if (i <= 3) { src = vb + (L->in_b - L->skip_b) + (i - 1) * 256 + c * R::S; d = R::IN_B + (i - 1) * R::S; n = R::S / 4; }
            else if (i <= 8) { const int64_t f = i == 4 ? L->n1w : i == 5 ? L->n1b : i == 6 ? L->l2b : i == 7 ? L->n2w : L->n2b; src = vpg + f; d = R::V5 + (i - 4) * 256; }
            else if (i == 9) { src = vpg + L->f1b; d = R::F1B; n = FF_D / 4; }
            else if (i <= 13) { const int64_t f = i == 10 ? L->f2b : i == 11 ? L->fsnw : i == 12 ? L->fsnb : L->fo_b; src = vpg + f; d = R::V4 + (i - 10) * 256; }
            else if (i <= 15) { src = A.ctab + (size_t)b * SEEME_CROW + l * 512 + (i - 14) * 256; d = R::CT + (i - 14) * 256; }
            else { src = vpg + L->l1b + c * R::NB + (i - 16) * 256; d = R::L1B + (i - 16) * 256; n = R::NB >= 256 ? 64 : R::NB / 4; }
            d += l * R::LAYER;
        }
        if (lane < n) lds_dma_1k(src + 4 * lane, base + (uint32_t)d * 4u);
    }
}
// one changing row of the NEXT layer per wave (waves 1 .. 5 hold rows 0 .. 4; waves 6, 7 request a row again and drop it, so that no branch
// stands around the load): all 64 lanes load, 4 registers live inside the X1 window only
struct ClRow {
    float4 r;
    __device__ __forceinline__ void load(int wave, int lane, const float* __restrict__ tt_row, const float* __restrict__ ca_row, int l) {
        const int j = wave - 1 - (wave > 5 ? 5 : 0);
        const float* src = j < 2 ? tt_row + l * 512 + j * 256 : (j < 4 ? tt_row + 2560 + l * 1024 + 512 + (j - 2) * 256 : ca_row);
        r = *reinterpret_cast<const float4*>(src + 4 * lane);
    }
    __device__ __forceinline__ void store(int wave, int lane, float* __restrict__ rows) const {
        if (wave >= 1 && wave <= 5) *reinterpret_cast<float4*>(rows + (wave - 1) * 256 + 4 * lane) = r;
    }
};

// Two wave groups: what the scheduler step reads travels the same way, in the rows that waves 6 and 7 used to drop -- wave 6: the 8 coefficients
// of THIS step (lanes read coef[step][4 (lane & 1) ..]), wave 7: the sample's row of step noise (when given) -- into COEF | NZ behind the window
// flags, and every wave reads the table row of the NEXT step (trow) for itself.  They are requested in the X1 window of EVERY layer (no branch
// around a request; the five windows of a step write the same values, and the step's closing barrier stands between the scheduler's reads and
// the next step's first window), so the scheduler step finds them in LDS and waits for no global load: before, it issued two dependent pairs
// of scalar loads behind the stack norm, the noise row was loaded at its use with vmcnt(0) -- draining the weight ring -- and the next row was a
// scalar load waited for at the top of the layer loop.  Without a scheduler (forward) / without noise the lanes re-read the row they dropped.
struct ClRowG {
    float4 r; int t;
    __device__ __forceinline__ void load(int wave, int lane, const float* __restrict__ tt_row, const float* __restrict__ ca_row, int l,
                                         const SeemeSampleArgs& A, int b, int step, int step_next) {
        int z = 0;
        asm volatile("" : "+v"(z));        // (a lane-dependent address in form: a vector load, counted by vmcnt like the row behind it)
        t = A.trow[(A.trow_per_sample ? b : step_next) + z];
        const int j = wave - 1 - (wave > 5 ? 5 : 0);
        const float* src = (j < 2 ? tt_row + l * 512 + j * 256 : (j < 4 ? tt_row + 2560 + l * 1024 + 512 + (j - 2) * 256 : ca_row)) + 4 * lane;
        if (wave == 6 && A.sched != SEEME_SCHED_NONE) src = A.coef + (size_t)step * 8 + 4 * (lane & 1);
        if (wave == 7 && A.noise != nullptr) src = sched_noise_row(A.noise, A.B, step, b, lane);
        r = *reinterpret_cast<const float4*>(src);
    }
    // one LDS write per wave: rows 0 .. 4 (waves 1 .. 5) | COEF (wave 6: every lane pair writes the same 8 floats) | NZ (wave 7); returns the next step's row
    __device__ __forceinline__ int store(int wave, int lane, float* __restrict__ rows, float* __restrict__ coef, float* __restrict__ nz) const {
        float* dst = wave == 6 ? coef + 4 * (lane & 1) : (wave == 7 ? nz + 4 * lane : rows + (wave - 1) * 256 + 4 * lane);
        *reinterpret_cast<float4*>(dst) = r;
        return __builtin_amdgcn_readfirstlane(t);
    }
};

template <int C, bool Q>
struct ClStage {
    float4 r; int dst, n4;        // ONE piece per wave and phase (Q: k = 0 .. 4 in phases B, C, H, D, F): 4 registers live across a phase
    static constexpr int NL1 = ClG<C, Q>::NB > 256 ? ClG<C, Q>::NB / 256 : 1;
    __device__ __forceinline__ void load(int k, int wave, int lane, const float* __restrict__ vpg, const DenLayerOff* __restrict__ L,
                                         const float* __restrict__ tt_row, int l, const SeemeSampleArgs& A, int b, int c, int ca_r, int ca_R) {
        typedef ClG<C, Q> G;
        const float* vb = vpg + L->skip_b;
        const int o_in = (int)(L->in_b - L->skip_b);
        const int i = wave + 8 * k;
        const float* src = vb; int d = 0, n = 0;
        if (i == 0) { d = c * G::S; src = vb + d; n = G::S / 4; }
        else if (i <= 3) { d = o_in + (i - 1) * 256 + c * G::S; src = vb + d; n = G::S / 4; }
        else if (i <= 13) {
            const int64_t f = i == 4 ? L->n1w : i == 5 ? L->n1b : i == 6 ? L->l2b : i == 7 ? L->n2w : i == 8 ? L->n2b : i == 9 ? L->f1b
                            : i == 10 ? L->f2b : i == 11 ? L->fsnw : i == 12 ? L->fsnb : L->fo_b;
            d = (int)(f - L->skip_b); src = vb + d; n = i == 9 ? FF_D / 4 : 64;
        }
        else if (i <= 15) { src = tt_row + l * 512 + (i - 14) * 256; d = VP_LAYER + (i - 14) * 256; n = 64; }                 // time token K | V'
        else if (i <= 17) { src = tt_row + 2560 + l * 1024 + 512 + (i - 16) * 256; d = VP_LAYER + 1024 + (i - 16) * 256; n = 64; }   // ffn AdaLN scale | shift
        else if (i < 18 + NL1) { d = (int)(L->l1b - L->skip_b) + c * G::NB + (i - 18) * 256; src = vb + d; n = G::NB >= 256 ? 64 : G::NB / 4; }
        else {
            const int j = i - 18 - NL1;
            if (j <= 1) { src = tt_row + 2560 + l * 1024 + j * 256; d = VP_LAYER + 512 + j * 256; n = 64; }                                 // ca AdaLN scale | shift
            else if (j <= 6) {
                const int64_t f = j == 2 ? L->cnw : j == 3 ? L->cnb : j == 4 ? L->csnw : j == 5 ? L->csnb : L->cao_b;
                d = (int)(f - L->skip_b); src = vb + d; n = 64;
            }
            else if (j == 7) { d = (int)(L->caq_b - L->skip_b) + c * G::S; src = vb + d; n = G::S / 4; }
            else if (j < 8 + 4 * A.N) {                // condition tokens: sa K | sa V' | ca key | ca value, 256 floats each
                const int t = (j - 8) >> 2, q = (j - 8) & 3;
                src = A.ctab + ((size_t)b * A.N + t) * SEEME_CROW + (q < 2 ? l * 512 + q * 256 : 2560 + l * 512 + (q - 2) * 256);
                d = VP_LAYER + STG_TT + t * 1024 + q * 256; n = 64;
            }
        }
        dst = d; n4 = n;
        r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < n) r = *reinterpret_cast<const float4*>(src + 4 * lane);
    }
    __device__ __forceinline__ void store(int lane, float* __restrict__ stg) const {
        if (lane < n4) *reinterpret_cast<float4*>(stg + dst + 4 * lane) = r;
    }
};
// pieces (Q): 26 + NL1 + 4 N <= 40 (five phases x 8 waves) for N <= 2 (C = 2: N = 2 gives 36)
#define DCL_MAX_N 2

template <typename WT, int C, bool Q>
__global__ __launch_bounds__(DEN_THREADS) void k_den_cluster(const ClArgs ka) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    typedef ClW<WT> W; typedef ClG<C, Q> G;
    // re-fills left until after the exchange: the last RU units of stage A (x half + skip half) and of stage C
    constexpr int A_DEF0 = cl_clamp(2 * G::TA - W::RU, 0, 2 * G::TA);          // first deferred unit of the 2 TA units of stage A
    constexpr int A_INL0 = cl_clamp(A_DEF0, 0, G::TA), A_INL1 = cl_clamp(A_DEF0 - G::TA, 0, G::TA), C_INL = cl_clamp(G::TB - W::RU, 0, G::TB);
    constexpr bool GRP = ClGrp<WT, C, Q>::ON;   // two wave groups: see ClGrp
    typedef std::conditional_t<GRP, ClSchedGrp, ClSched<C, WT::MFMA, Q>> SCH;
    constexpr bool WIN = SCH::WIN;       // (then stages A .. E request nothing inline: the windows do)
    const SeemeSampleArgs& A = ka.s;
    const DenLayout* __restrict__ lay = &ka.lay;
    const float* __restrict__ vp = ka.vp;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // which sample, which part of it: placement 0 = the cluster's workgroups have equal blockIdx % 8 (one XCD under
    // round-robin dispatch), placement 1 = consecutive blockIdx (C different XCDs).  Speed only.
    int b, c;
    if (ka.placement == 0) { const int x = blockIdx.x & 7, j = blockIdx.x >> 3; b = x * (ka.clusters / 8) + j / C; c = j % C; }
    else { b = blockIdx.x / C; c = blockIdx.x % C; }
    if (b >= A.B) return;                                      // (whole clusters: every member sees the same b)
    const bool epi = wave == 0;
    const int N = Q ? A.N : 1;
    typedef ClRes<C> R;
    constexpr bool RSD = !Q;                     // launch-constant operands resident in LDS (ClRes); Q: per-layer staging (ClStage)
    const int stg_sz = VP_LAYER + STG_TT + N * 1024;             // (Q) one half of the staging buffer, full layout
    const int ca_R = A.trow_per_sample ? 1 : A.steps;

    float* CONSTV = smem;                        // [768]  query_pos.pe[0], encoder.norm.{weight,bias}
    float* KEEP = CONSTV + 768;                  // [256]  the latent (epilogue wave)
    float* STG = KEEP + 256;                     // RSD: [5][R::LAYER] resident operands | [2][R::ROWS] changing rows;  Q: [2][stg_sz] per-layer operands
    float* ROWS = STG + SEEME_DEN_NL * R::LAYER; // (RSD)
    float* XA = STG + (RSD ? R::FLOATS : 2 * stg_sz);   // [512]  GEMV input: layer input x / x2   (16-bit: fragments of 256 k = 2 KiB)
    float* XB = XA + 512;                        // [512]  GEMV input: x1 / u
    float* XH = XB + 512;                        // [2 NB] GEMV input: this CU's hidden units / ffn hidden (fragments of NB k)
    float* SKF = XH + 2 * (G::NB > 128 ? G::NB : 128);   // [2][512] outputs of layers 0, 1 (skip inputs of layers 4, 3)
    float* QS = SKF + 1024;                      // [S] q, [S] k of this CU's dims
    float* KS = QS + G::S;
    float* PART = KS + G::S;                     // [256]
    float* RES = PART + 256;                     // [256]  the fp32 residual stream
    int* FLG = reinterpret_cast<int*>(RES + 256);   // [4]
    float* COEF = RES + 256 + 4;                 // (GRP) [8]   the step's scheduler coefficients (+ 4 spare), see ClRowG
    float* NZ = COEF + 12;                       // (GRP) [256] the sample's step noise
    int* FPI = reinterpret_cast<int*>(COEF + 8); // (GRP) "first poll issued": the exchange's epoch (the first of COEF's spare words; FLG has none)
    constexpr int XZERO = 512 + 512 + 2 * (G::NB > 128 ? G::NB : 128) + 1024;

    const __amdgpu_buffer_rsrc_t wg = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ka.wgc), 0, (int)ka.wgc_bytes, 0x00020000);
    unsigned long long* const xg = ka.xg + (size_t)b * G::G_TOTAL;
    const __amdgpu_buffer_rsrc_t xr_ = __builtin_amdgcn_make_buffer_rsrc(xg, 0, G::G_TOTAL * 8, 0x00020000);
    const unsigned voff = (unsigned)wave * (unsigned)(W::UL * 1024) + (unsigned)lane * 16u;
    const int w4 = wave & 3;                     // (GRP) the stored waves this wave plays: w4, w4 + 4
    const unsigned gvoff = (unsigned)w4 * (unsigned)(W::UL * 1024) + (unsigned)lane * 16u;
    const int col = lane & 15;
    const ClX xa = cl_xin<WT>(XA, lane), xb = cl_xin<WT>(XB, lane), xh = cl_xin<WT>(XH, lane);
    const float sa_scale = 1.f / 16.f;           // one head of 256 dims
    if (epi) __builtin_amdgcn_s_setprio(3);

    typedef const __attribute__((address_space(4))) int32_t* CI32;
    const CI32 trow_c = (CI32)(uintptr_t)A.trow;
    int row = A.trow_per_sample ? trow_c[b] : trow_c[0];

    // ---- prologue: constants, small operands (resident: all layers; Q: layer 0), zeroed fragment buffers, first input, first RU units, the XCC census
    float4 xr = ld4(A.latents + (size_t)b * 256 + 4 * lane);
    for (int i = tid; i < 192; i += DEN_THREADS)
        st4(CONSTV + 4 * i, i < 64 ? ld4(vp + lay->pe0 + 4 * i) : (i < 128 ? ld4(vp + lay->fnw + 4 * (i - 64)) : ld4(vp + lay->fnb + 4 * (i - 128))));
    if constexpr (RSD) cl_load_resident<C>(wave, lane, STG, vp, lay, A.ttab + (size_t)row * SEEME_TROW, A, b, c, ca_R);
    else stage_dma<1, Q, 0, 0>(wave, lane, STG, vp, &lay->L[0], A.ttab + (size_t)row * SEEME_TROW, 0, A, b, N, 0, ca_R);
    for (int i = tid; i < XZERO / 4; i += DEN_THREADS) st4(XA + 4 * i, make_float4(0.f, 0.f, 0.f, 0.f));
    if (tid >= 1 && tid < 4) FLG[tid] = 0;                   // window flags (epochs are never 0)
    if constexpr (GRP) { if (tid == 4) FPI[0] = 0; }
    bool dead = false, local = false;
    if (epi) {
        // first exchange, always write-through: the XCC id of every workgroup of the cluster (HW_REG_XCC_ID, bits 3:0)
        const unsigned my_xcc = __builtin_amdgcn_s_getreg(0x1814) & 15u;
        if (lane == 0) cl_store_granule(xg + G::G_BOOT + c, DCL_MAGIC_EPOCH, __uint_as_float(my_xcc), false);
        unsigned spins = 0, idv = 0;
        for (;;) {
            const unsigned long long x = __hip_atomic_load((dcl_gu64*)(xg + G::G_BOOT + (lane % C)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            idv = (unsigned)x;
            if (__all((unsigned)(x >> 32) == DCL_MAGIC_EPOCH)) break;
            if (++spins > DCL_SPIN_LIMIT) { dead = true; if (lane == 0) atomicOr(ka.hdr, 1u); break; }
            __builtin_amdgcn_s_sleep(2);
        }
        local = !dead && __all(idv == my_xcc) && !(ka.flags & 1);
        if (lane == 0) { FLG[0] = local ? 1 : 0; if (local && c == 0) atomicAdd(ka.hdr + 1, 1u); }
    }
    wait_vmcnt0();
    __syncthreads();
    local = FLG[0] != 0;
    if (epi) {
        st4(KEEP + 4 * lane, xr);
        xr = f4_add(xr, ld4(CONSTV + 4 * lane));                // sample + query_pos (mld_denoiser.py:210)
        put_x<WT, 1>(XA, 0, 0, lane, xr);
        st4(RES + 4 * lane, xr);
    }
    ClRing<WT> ring;
    ClRing2 gr;                                  // (GRP)
    (void)gr; (void)gvoff; (void)w4; (void)COEF; (void)NZ; (void)FPI;
    if constexpr (GRP) {
        if (wave < 4) {       // layer 0 has no skip linear; A1 is requested all the same (nowhere), as after every phase F: one count of loads in flight at a layer's start
            clg_issue<0>(gr, gvoff, wg, (unsigned)(c * G::NU + G::U_A) * W::UNIT_BYTES, true, w4 < 2);
            clg_issue<1>(gr, gvoff, wg, (unsigned)(c * G::NU + G::U_AS) * W::UNIT_BYTES, false, false);
        }
    } else {
        const unsigned b0 = (unsigned)((0 * C + c) * G::NU) * W::UNIT_BYTES;
        cl_issue<WT, C, Q, 0>(ring, wave, voff, wg, b0, b0, false, false);
        cl_issue<WT, C, Q, 1>(ring, wave, voff, wg, b0, b0, false, false);
        if constexpr (W::RU == 4 && (!WIN || SCH::PRO == 4)) { cl_issue<WT, C, Q, 2>(ring, wave, voff, wg, b0, b0, false, false); cl_issue<WT, C, Q, 3>(ring, wave, voff, wg, b0, b0, false, false); }
    }
    __syncthreads();
    int cur = 0;
    int row_nx = row;                            // (GRP) table row of the next step, as this wave last read it
    (void)row_nx;

#pragma unroll 1
    for (int step = 0; step < A.steps; ++step) {
        if (step == 2) DEN_DBG(1);
        if (step == 3) DEN_DBG(2);
        const int step_next = step + 1 < A.steps ? step + 1 : step;
        // the table row of the next step: a scalar load here, waited for at the top of the layer loop -- or (GRP) read by every wave for itself
        // in the X1 windows (ClRowG; row_nx as of layer 3's window when layer 4's asks for it)
        int row_next = row;
        if constexpr (!GRP) row_next = A.trow_per_sample ? row : trow_c[step_next];
#pragma unroll 1
        for (int l = 0; l < SEEME_DEN_NL; ++l) {
            const DenLayerOff* __restrict__ L = &lay->L[l];
            const int ln = (l + 1 < SEEME_DEN_NL) ? l + 1 : 0;
            const DenLayerOff* __restrict__ Ln = &lay->L[ln];
            const bool skip = l >= 3, nskip = ln >= 3;
            const unsigned bc = (unsigned)((l * C + c) * G::NU) * W::UNIT_BYTES, bn = (unsigned)((ln * C + c) * G::NU) * W::UNIT_BYTES;
            // small operands: layer l of the resident block + the current half of the changing rows (RSD), or the current half of the
            // staging buffer in the layout of the vector-parameter image (Q).  v_skip_b, v_in_b and v_l1b hold this CU's slices only
            // when resident: IN_ST = distance of the q, k, v' parts of in_b, d0 / j0 = this CU's first dim / hidden unit in them.
            const float* VP = STG + (RSD ? l * R::LAYER : cur * stg_sz);
            const float* TTS = RSD ? ROWS + cur * R::ROWS : VP + VP_LAYER;        // time token K | V' ...
            const float* TFS = TTS + (RSD ? 512 : 1024);                          // ... ffn AdaLN scale | shift
            const float* CT = RSD ? VP + R::CT : TTS + STG_TT;
            const float* CA_ADD = TTS + 1024;                                     // (RSD) the tabulated ca term
            constexpr int IN_ST = RSD ? G::S : 256;
            const int d0 = RSD ? 0 : c * G::S, j0 = RSD ? 0 : c * G::NB;
            const float* v_skip_b = RSD ? VP + R::SKIP_B : VP;
            const float* v_in_b = RSD ? VP + R::IN_B : VP + (L->in_b - L->skip_b);
            const float* v_n1w = RSD ? VP + R::V5 : VP + (L->n1w - L->skip_b), *v_n1b = RSD ? VP + R::V5 + 256 : VP + (L->n1b - L->skip_b);
            const float* v_l1b = RSD ? VP + R::L1B : VP + (L->l1b - L->skip_b), *v_l2b = RSD ? VP + R::V5 + 512 : VP + (L->l2b - L->skip_b);
            const float* v_n2w = RSD ? VP + R::V5 + 768 : VP + (L->n2w - L->skip_b), *v_n2b = RSD ? VP + R::V5 + 1024 : VP + (L->n2b - L->skip_b);
            const float* v_f1b = RSD ? VP + R::F1B : VP + (L->f1b - L->skip_b), *v_f2b = RSD ? VP + R::V4 : VP + (L->f2b - L->skip_b);
            const float* v_fsnw = RSD ? VP + R::V4 + 256 : VP + (L->fsnw - L->skip_b), *v_fsnb = RSD ? VP + R::V4 + 512 : VP + (L->fsnb - L->skip_b);
            const float* v_fo_b = RSD ? VP + R::V4 + 768 : VP + (L->fo_b - L->skip_b);
            const float* v_cnw = VP + (L->cnw - L->skip_b), *v_cnb = VP + (L->cnb - L->skip_b), *v_caq_b = VP + (L->caq_b - L->skip_b);
            const float* v_csnw = VP + (L->csnw - L->skip_b), *v_csnb = VP + (L->csnb - L->skip_b), *v_cao_b = VP + (L->cao_b - L->skip_b);
            (void)CA_ADD; (void)v_cnw; (void)v_cnb; (void)v_caq_b; (void)v_csnw; (void)v_csnb; (void)v_cao_b;
            const bool ywave = wave >= 6;
            // the next layer's changing operands: table row of the next step behind the last layer
            const float* const tt_next = A.ttab + (size_t)(ln == 0 ? (GRP ? row_nx : row_next) : row) * SEEME_TROW;
            const int ca_next = A.trow_per_sample ? 0 : (ln == 0 ? step_next : step);
            ClStage<C, true> nxt;       // (Q)
            (void)nxt; (void)ca_next;
            const unsigned e1 = 1u + (unsigned)G::EPL * (unsigned)(step * SEEME_DEN_NL + l), e2 = e1 + 1u, e3 = e1 + 2u;   // epochs of this layer's exchanges
            (void)e3;

            if constexpr (GRP) {
                if (wave >= 4) {
                    // ======== group G1: phases B, D, F; the same barriers as G0 below, which runs A, C, E and the epilogue wave's parts ========
                    __syncthreads();                                                   // A
                    {   // X1 published: the next layer's changing row (oldest load, see ClRow), then unit B
                        ClRowG nrow;
                        cl_flag_wait(FLG + 1, e1);
                        nrow.load(wave, lane, tt_next, A.catab + (((size_t)b * ca_R + ca_next) * SEEME_DEN_NL + ln) * 256, ln, A, b, step, step_next);
                        __builtin_amdgcn_sched_barrier(0);
                        clg_issue<0>(gr, gvoff, wg, bc + (unsigned)G::U_B * W::UNIT_BYTES, true, true);
                        row_nx = nrow.store(wave, lane, ROWS + (cur ^ 1) * R::ROWS, COEF, NZ);
                    }
                    __syncthreads();                                                   // X1
                    {   // B: linear1 + ReLU
                        f32x4 acc[2][1];
                        uint4 fr[8];
                        const int j = (w4 + 4 * ((lane >> 4) & 1)) * 16 + col;
                        clg_frags<8>(fr, xb);
                        const float bias = v_l1b[j];                                   // ahead of the MFMAs: no LDS round trip behind them
                        __builtin_amdgcn_sched_barrier(0);
                        cl_zero<1>(acc[0]); cl_zero<1>(acc[1]);
                        clg_consume<WT, 1, 8, 0>(gr.r[0], fr, acc);
                        cl_pin<1>(acc[0]); cl_pin<1>(acc[1]);
                        if (lane < 32) cl_put1<WT>(XH, j, fmaxf(clg_out<WT, 1>(acc, lane) + bias, 0.f));
                    }
                    __syncthreads();                                                   // B
                    cl_flag_wait(FLG + 1, e2);                                         // X2 published: D
                    clg_issue<1>(gr, gvoff, wg, bc + (unsigned)G::U_D * W::UNIT_BYTES, true, true);
                    cl_flag_wait(FLG + 2, e2);                                         // X2 swept: F0
                    clg_issue<0>(gr, gvoff, wg, bc + (unsigned)G::U_F * W::UNIT_BYTES, true, true);
                    __syncthreads();                                                   // C + X2
                    {   // D: ffn.linear1 + GELU
                        f32x4 acc[2][1];
                        uint4 fr[8];
                        const int j = (w4 + 4 * ((lane >> 4) & 1)) * 16 + col;
                        clg_frags<8>(fr, xa);
                        const float bias = v_f1b[j];
                        __builtin_amdgcn_sched_barrier(0);
                        cl_zero<1>(acc[0]); cl_zero<1>(acc[1]);
                        clg_consume<WT, 1, 8, 0>(gr.r[1], fr, acc);
                        cl_pin<1>(acc[0]); cl_pin<1>(acc[1]);
                        if (lane < 32) cl_put1<WT>(XH, j, fast_gelu(clg_out<WT, 1>(acc, lane) + bias));
                    }
                    __syncthreads();                                                   // D
                    // F1 in two halves, phase E and the ffn epilogue: the 64 wave-loads of a whole unit take the address path longer than phase E lasts,
                    // and the barrier that ends a phase waits for the requesting group as well
                    clg_issue<1, 1>(gr, gvoff, wg, bc + (unsigned)(G::U_F + 1) * W::UNIT_BYTES, true, true);
                    __syncthreads();                                                   // E
                    clg_issue<1, 2>(gr, gvoff, wg, bc + (unsigned)(G::U_F + 1) * W::UNIT_BYTES, true, true);
                    __syncthreads();                                                   // ffn epilogue
                    {   // F: ffn.proj_out.out_layers + residual; writes the next layer's input
                        f32x4 acc[2][2];
                        uint4 fr[8];
                        const int n = (2 * (w4 + 4 * (lane >> 5)) + ((lane >> 4) & 1)) * 16 + col;
                        clg_frags<8>(fr, xb);
                        const float res = RES[n], bias = v_fo_b[n];                    // (RES: final since norm2, three barriers back)
                        __builtin_amdgcn_sched_barrier(0);
                        cl_zero<2>(acc[0]); cl_zero<2>(acc[1]);
                        clg_consume<WT, 2, 8, 0>(gr.r[0], fr, acc);
                        cl_pin<2>(acc[0]); cl_pin<2>(acc[1]);
                        clg_consume<WT, 2, 8, 4>(gr.r[1], fr, acc);
                        cl_pin<2>(acc[0]); cl_pin<2>(acc[1]);
                        const float xn = res + clg_out<WT, 2>(acc, lane) + bias;
                        RES[n] = xn;
                        cl_put1<WT>(XA, n, xn);
                        if (l < 2) cl_put1<WT>(SKF + 512 * l, n, xn);
                    }
                    __syncthreads();                                                   // F
                    if (l + 1 == SEEME_DEN_NL) __syncthreads();                        // stack norm, scheduler step
                    cur ^= 1;
                    continue;
                }
            }

            // ================= A: in_proj' (+ folded skip linear), column-split by dims =================
            if constexpr (GRP) {
                // Fragments of the layer input and the lane's bias go out ahead of the first MFMA, those of the skip input (second k-half: final
                // since layers 0 / 1; read in every layer, used where the layer has a skip linear) into the registers the first k-half frees.
                // Lane epilogue: stored wave = tile; waves 0,1: q; 2,3: k; 4,5: v'; 6,7: y -- this wave plays w4 in lanes 0 .. 15 (q or k -> LDS)
                // and w4 + 4 in lanes 16 .. 31 (v', or y where the layer has a skip linear -> granule): one bias read ahead of the chain, one
                // add, one store of either kind instead of four nested sections with a read each.  The granule goes first: peers wait for it.
                f32x4 acc[2][1];
                uint4 fr[8];
                const bool hi = (lane & 16) != 0, qv = w4 < 2;
                const int d = (w4 & 1) * 16 + col;
                const float* bsrc = hi ? (qv ? v_in_b + 2 * IN_ST : v_skip_b) : (qv ? v_in_b : v_in_b + IN_ST);
                clg_frags<8>(fr, xa);
                const float bias = bsrc[d];
                __builtin_amdgcn_sched_barrier(0);
                cl_zero<1>(acc[0]); cl_zero<1>(acc[1]);
                clg_consume_refill<WT>(gr.r[0], fr, cl_xin<WT>(SKF + (l == 3 ? 512 : 0), lane), acc);
                cl_pin<1>(acc[0]); cl_pin<1>(acc[1]);
                if (skip) clg_consume<WT, 1, 8, 0>(gr.r[1], fr, acc);
                cl_pin<1>(acc[0]); cl_pin<1>(acc[1]);
                const float val = clg_out<WT, 1>(acc, lane) + bias;
                if (hi && lane < 32 && (qv || skip)) cl_store_granule(xg + G::G_X1 + c * G::X1_G + (qv ? 0 : G::S) + d, e1, val, local);
                if (lane < 16) (qv ? QS : KS)[d] = val;
            } else {
                f32x4 acc[G::TA];
                cl_zero<G::TA>(acc);
                const bool act = skip || !ywave;
                cl_units<WT, C, Q, G::U_A, G::TA, G::TA, 0, 0, A_INL0>(ring, xa, acc, act, wave, voff, wg, bc, bn, skip, nskip, std::make_integer_sequence<int, G::TA>{});
                {   // second k-half: the skip input (output of layer 1 for layer 3, of layer 0 for layer 4: xs.pop(), cross_attention.py:77-79)
                    const ClX xs = cl_xin<WT>(SKF + (l == 3 ? 512 : 0), lane);
                    cl_units<WT, C, Q, G::U_AS, G::TA, G::TA, G::TA, W::UL, A_INL1>(ring, xs, acc, skip, wave, voff, wg, bc, bn, skip, nskip, std::make_integer_sequence<int, G::TA>{});
                }
                if (act && lane < 16) {
#pragma unroll
                    for (int t = 0; t < G::TA; ++t) {
                        const int T = wave * G::TA + t, part = T / (G::S / 16), d = (T % (G::S / 16)) * 16 + col, D = d0 + d;
                        const float val = cl_out<WT>(acc[t]);
                        const unsigned epoch = e1;
                        if (part == 0) QS[d] = val + v_in_b[D];
                        else if (part == 1) KS[d] = val + v_in_b[IN_ST + D];
                        else if (part == 2) cl_store_granule(xg + G::G_X1 + c * G::X1_G + d, epoch, val + v_in_b[2 * IN_ST + D], local);
                        else cl_store_granule(xg + G::G_X1 + c * G::X1_G + G::S + d, epoch, val + v_skip_b[D], local);
                    }
                }
            }
            __syncthreads(); DEN_DBG(0);
            if (epi) {
                // partial scores over this CU's dims: token 0 itself, the condition token(s), the time token (last; mdiff_transformer.py:295)
                const unsigned epoch = e1;
                constexpr int NT = Q ? DCL_MAX_N + 2 : 3;          // score slots: [0] self, [1 .. N] condition, [N + 1] time
                float ps[NT];
#pragma unroll
                for (int j = 0; j < NT; ++j) ps[j] = 0.f;
#pragma unroll
                for (int dd = 0; dd < G::S; dd += 64) {
                    const int d = dd + lane;
                    if (d < G::S) {
                        const float q = QS[d];
                        ps[0] = fmaf(q, KS[d], ps[0]);
#pragma unroll
                        for (int n = 0; n < NT - 2; ++n) if (n < N) ps[1 + n] = fmaf(q, CT[n * 1024 + c * G::S + d], ps[1 + n]);
                        ps[NT - 1] = fmaf(q, TTS[c * G::S + d], ps[NT - 1]);
                    }
                }
#pragma unroll
                for (int j = 0; j < NT; ++j) ps[j] = wave_sum(ps[j]) * sa_scale;
                {
                    float pv = 0.f;
#pragma unroll
                    for (int j = 0; j < NT; ++j) pv = lane == j ? ps[j] : pv;
                    if (lane < G::SC) cl_store_granule(xg + G::G_X1 + c * G::X1_G + 2 * G::S + lane, epoch, pv, local);
                }
                if constexpr (WIN) {        // published: this wave's share of W1A, then the others'; the first poll waits until the unit has drained
                    __builtin_amdgcn_sched_barrier(0);
                    cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::W1A{});
                    if (lane == 0) cl_flag_set(FLG + 1, e1);
                    __builtin_amdgcn_s_sleep(DCL_POLL_SLEEP);
                }
                // ---- X1: gather v' (and y), all-reduce the scores
                const int pub = (4 * lane) / G::S, off = (4 * lane) % G::S;
                const unsigned o_v = (unsigned)((G::G_X1 + pub * G::X1_G + off) * 8);
                const unsigned o_s = (unsigned)((G::G_X1 + (lane % C) * G::X1_G + 2 * G::S) * 8);
                u32x4 gv0, gv1, gy0, gy1, gs[G::SC / 2];
                gy0 = gy1 = u32x4{0u, epoch, 0u, epoch};
                unsigned spins = 0;
                bool swept = false;
                if constexpr (GRP) {
                    // The FIRST poll, peeled: behind its loads the vector-memory path has nothing to do until they return, and waves 1 .. 3 spin.
                    // The first half of unit E (stored waves 0 .. 3) goes out in that flight time -- this wave's share first (behind the others' it
                    // would wait out their backlog), then the release of waves 1 .. 3 (FPI) -- and the poll is checked with the loads still in
                    // flight: the poll's are the older ones, vmcnt(8 + ...).  (The loads and the check stand here and in the loop below in full: shared
                    // through lambdas, every instantiation's poll loop compiled differently -- five-fold unrolled, five more vmcnt(0).)  A poll that has to be repeated stands behind them (and waits with
                    // vmcnt(0)), which is why only half a unit travels here: the whole unit cost X1 0.7 k cycles for 0.35 k off phase B, the half
                    // 0.2 k for 0.35 k (profiles/cluster_poll_windows.txt); the other half stays in phase B, which hides 32 wave-loads.
                    gv0 = __builtin_amdgcn_raw_buffer_load_b128(xr_, o_v, 0, 16);
                    gv1 = __builtin_amdgcn_raw_buffer_load_b128(xr_, o_v + 16, 0, 16);
                    if (skip) {
                        gy0 = __builtin_amdgcn_raw_buffer_load_b128(xr_, o_v + G::S * 8, 0, 16);
                        gy1 = __builtin_amdgcn_raw_buffer_load_b128(xr_, o_v + G::S * 8 + 16, 0, 16);
                    }
#pragma unroll
                    for (int j = 0; j < G::SC / 2; ++j) gs[j] = __builtin_amdgcn_raw_buffer_load_b128(xr_, o_s + 16 * j, 0, 16);
                    __builtin_amdgcn_sched_barrier(0);
                    clg_issue<1, 1>(gr, gvoff, wg, bc + (unsigned)G::U_E * W::UNIT_BYTES, true, true);
                    if (lane == 0) cl_flag_set(FPI, e1);
                    __builtin_amdgcn_sched_barrier(0);
                    unsigned ok = cl_tags_ok(gv0, epoch) & cl_tags_ok(gv1, epoch) & cl_tags_ok(gy0, epoch) & cl_tags_ok(gy1, epoch);
#pragma unroll
                    for (int j = 0; j < G::SC / 2; ++j) ok &= cl_tags_ok(gs[j], epoch);
                    swept = __all(ok != 0u) || dead;
                    asm volatile("" ::: "memory");      // (a later poll reads the granules again)
                }
                if (!swept) for (;;) {
                    gv0 = __builtin_amdgcn_raw_buffer_load_b128(xr_, o_v, 0, 16);
                    gv1 = __builtin_amdgcn_raw_buffer_load_b128(xr_, o_v + 16, 0, 16);
                    if (skip) {
                        gy0 = __builtin_amdgcn_raw_buffer_load_b128(xr_, o_v + G::S * 8, 0, 16);
                        gy1 = __builtin_amdgcn_raw_buffer_load_b128(xr_, o_v + G::S * 8 + 16, 0, 16);
                    }
#pragma unroll
                    for (int j = 0; j < G::SC / 2; ++j) gs[j] = __builtin_amdgcn_raw_buffer_load_b128(xr_, o_s + 16 * j, 0, 16);
                    unsigned ok = cl_tags_ok(gv0, epoch) & cl_tags_ok(gv1, epoch) & cl_tags_ok(gy0, epoch) & cl_tags_ok(gy1, epoch);
#pragma unroll
                    for (int j = 0; j < G::SC / 2; ++j) ok &= cl_tags_ok(gs[j], epoch);
                    if (__all(ok != 0u) || dead) break;
                    if (++spins > DCL_SPIN_LIMIT) { dead = true; if (lane == 0) atomicOr(ka.hdr, 2u); break; }
                }
                if constexpr (WIN) {
                    cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::W1B{});
                    if constexpr (GRP) clg_issue<0>(gr, gvoff, wg, bc + (unsigned)G::U_C * W::UNIT_BYTES, true, true);
                    if (lane == 0) cl_flag_set(FLG + 2, e1);
                }
                DEN_DBG(0);
                float sc[NT];
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    sc[j] = __uint_as_float((j & 1) ? gs[j >> 1].z : gs[j >> 1].x);
                    // sum over the C publishers (aligned groups of C lanes hold one each): butterfly, the same order on every CU
                    if (C >= 2) sc[j] += dpp_f(sc[j], 0);
                    if (C >= 4) sc[j] += dpp_f(sc[j], 1);
                    if (C >= 8) sc[j] += dpp_f(sc[j], 2);
                }
                float mx = fmaxf(sc[0], sc[NT - 1]);
#pragma unroll
                for (int n = 0; n < NT - 2; ++n) if (n < N) mx = fmaxf(mx, sc[1 + n]);
                float esum = 0.f;
#pragma unroll
                for (int j = 0; j < NT; ++j) { sc[j] = (j == 0 || j == NT - 1 || j - 1 < N) ? fast_exp(sc[j] - mx) : 0.f; esum += sc[j]; }
                const float inv = fast_rcp(esum);
                const float4 vv = make_float4(__uint_as_float(gv0.x), __uint_as_float(gv0.z), __uint_as_float(gv1.x), __uint_as_float(gv1.z));
                float4 att = f4_scale(vv, sc[0] * inv);
#pragma unroll
                for (int n = 0; n < NT - 2; ++n) if (n < N) att = f4_fma(sc[1 + n] * inv, ld4(CT + n * 1024 + 256 + 4 * lane), att);
                att = f4_fma(sc[NT - 1] * inv, ld4(TTS + 256 + 4 * lane), att);
                if (skip) xr = make_float4(__uint_as_float(gy0.x), __uint_as_float(gy0.z), __uint_as_float(gy1.x), __uint_as_float(gy1.z));
                xr = wave_ln(f4_add(xr, att), v_n1w, v_n1b, lane);        // the "values" carry out_proj: residual + norm1
                put_x<WT, 1>(XB, 0, 0, lane, xr);
            } else {
                // the next layer's changing row first: the OLDEST load of the window.  It is stored behind the window's units, in front of the
                // barrier at which these waves wait out the epilogue wave's sweep and vector algebra anyway: the store's wait is
                // vmcnt(units requested behind the row) -- it leaves every unit in flight and the row has had the whole exchange to land.
                std::conditional_t<GRP, ClRowG, ClRow> nrow;
                if constexpr (WIN) cl_flag_wait(FLG + 1, e1);
                if constexpr (GRP) {
                    nrow.load(wave, lane, tt_next, A.catab + (((size_t)b * ca_R + ca_next) * SEEME_DEN_NL + ln) * 256, ln, A, b, step, step_next);
                    __builtin_amdgcn_sched_barrier(0);
                } else if constexpr (RSD) {
                    nrow.load(wave, lane, tt_next, A.catab + (((size_t)b * ca_R + ca_next) * SEEME_DEN_NL + ln) * 256, ln);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (WIN) {
                    cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::W1A{});
                    if constexpr (GRP) {     // the first poll is on its way: E's first half into its flight time (slot 1: phase A has consumed A1)
                        cl_flag_wait(FPI, e1);
                        clg_issue<1, 1>(gr, gvoff, wg, bc + (unsigned)G::U_E * W::UNIT_BYTES, true, true);
                    }
                    cl_flag_wait(FLG + 2, e1);
                    cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::W1B{});
                    if constexpr (GRP) clg_issue<0>(gr, gvoff, wg, bc + (unsigned)G::U_C * W::UNIT_BYTES, true, true);
                }
                if constexpr (GRP) row_nx = nrow.store(wave, lane, ROWS + (cur ^ 1) * R::ROWS, COEF, NZ);
                else if constexpr (RSD) nrow.store(wave, lane, ROWS + (cur ^ 1) * R::ROWS);
            }
            __syncthreads(); DEN_DBG(0);

            // ================= B: linear1 + ReLU, column-split =================
            // (Q: a piece of the next layer's small operands is requested here and stored to the other half of the staging buffer at the end
            //  of the phase -- BEFORE the deferred re-fills: vmcnt is in order, and the store must not wait for them)
            if constexpr (Q) nxt.load(0, wave, lane, vp, Ln, tt_next, ln, A, b, c, ca_next, ca_R);
            if constexpr (!WIN) cl_refills<WT, C, Q, G::U_A + A_DEF0>(ring, wave, voff, wg, bc, bn, skip, nskip, std::make_integer_sequence<int, 2 * G::TA - A_DEF0>{});   // slots of stage A
            if constexpr (GRP) {      // (G1 computes; this group requests E's second half: the first went out behind X1's first poll)
                clg_issue<1, 2>(gr, gvoff, wg, bc + (unsigned)G::U_E * W::UNIT_BYTES, true, true);
            } else {
                f32x4 acc[G::TB];
                cl_zero<G::TB>(acc);
                cl_units<WT, C, Q, G::U_B, G::TB, G::TB, 0, 0, (WIN ? 0 : G::TB)>(ring, xb, acc, true, wave, voff, wg, bc, bn, skip, nskip, std::make_integer_sequence<int, G::TB>{});
                if (lane < 16) {
#pragma unroll
                    for (int t = 0; t < G::TB; ++t) {
                        const int j = (wave * G::TB + t) * 16 + col;
                        cl_put1<WT>(XH, j, fmaxf(cl_out<WT>(acc[t]) + v_l1b[j0 + j], 0.f));
                    }
                }
            }
            if constexpr (Q) nxt.store(lane, STG + (cur ^ 1) * stg_sz);
            __syncthreads(); DEN_DBG(0);

            // ================= C: linear2, row-split -> X2 =================
            if constexpr (Q) nxt.load(1, wave, lane, vp, Ln, tt_next, ln, A, b, c, ca_next, ca_R);
            if constexpr (GRP) {
                f32x4 acc[2][2];
                uint4 fr[4];
                clg_frags<4>(fr, xh);
                __builtin_amdgcn_sched_barrier(0);
                cl_zero<2>(acc[0]); cl_zero<2>(acc[1]);
                clg_consume<WT, 2, 4, 0>(gr.r[0], fr, acc);
                cl_pin<2>(acc[0]); cl_pin<2>(acc[1]);
                cl_store_granule(xg + G::G_X2 + c * 256 + (2 * (w4 + 4 * (lane >> 5)) + ((lane >> 4) & 1)) * 16 + col, e2, clg_out<WT, 2>(acc, lane), local);
            } else {
                f32x4 acc[2];
                cl_zero<2>(acc);
                cl_units<WT, C, Q, G::U_C, G::TB, 2, 0, 0, C_INL>(ring, xh, acc, true, wave, voff, wg, bc, bn, skip, nskip, std::make_integer_sequence<int, G::TB>{});
                if (lane < 32) {
                    const float val = (lane & 16) ? cl_out<WT>(acc[1]) : cl_out<WT>(acc[0]);
                    cl_store_granule(xg + G::G_X2 + c * 256 + (2 * wave + (lane >> 4)) * 16 + col, e2, val, local);
                }
            }
            if constexpr (Q) nxt.store(lane, STG + (cur ^ 1) * stg_sz);
            if (epi) {
                const unsigned epoch = e2;
                if constexpr (WIN) {
                    __builtin_amdgcn_sched_barrier(0);
                    cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::W2A{});
                    if (lane == 0) cl_flag_set(FLG + 1, e2);
                    __builtin_amdgcn_s_sleep(DCL_POLL_SLEEP);
                }
                float4 sum;
                unsigned spins = 0;
                for (;;) {
                    u32x4 g[C][2];
#pragma unroll
                    for (int p = 0; p < C; ++p) {
                        const unsigned o = (unsigned)((G::G_X2 + p * 256 + 4 * lane) * 8);
                        g[p][0] = __builtin_amdgcn_raw_buffer_load_b128(xr_, o, 0, 16);
                        g[p][1] = __builtin_amdgcn_raw_buffer_load_b128(xr_, o + 16, 0, 16);
                    }
                    unsigned ok = 1u;
                    sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int p = 0; p < C; ++p) {
                        ok &= cl_tags_ok(g[p][0], epoch) & cl_tags_ok(g[p][1], epoch);
                        sum.x += __uint_as_float(g[p][0].x); sum.y += __uint_as_float(g[p][0].z);
                        sum.z += __uint_as_float(g[p][1].x); sum.w += __uint_as_float(g[p][1].z);
                    }
                    if (__all(ok != 0u) || dead) break;
                    if (++spins > DCL_SPIN_LIMIT) { dead = true; if (lane == 0) atomicOr(ka.hdr, 4u); break; }
                }
                if constexpr (WIN) {
                    cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::W2B{});
                    if (lane == 0) cl_flag_set(FLG + 2, e2);
                }
                DEN_DBG(0);
                // + bias, residual, norm2
                xr = wave_ln(f4_add(xr, f4_add(sum, ld4(v_l2b + 4 * lane))), v_n2w, v_n2b, lane);
                if constexpr (!Q) {
                    // ONE condition token: x + Stylization(v) does not depend on x (seeme_denoiser_ca_tables)
                    xr = f4_add(xr, ld4(CA_ADD + 4 * lane));
                    put_x<WT, 1>(XA, 0, 0, lane, xr);
                } else {
                    put_x<WT, 1>(XB, 0, 0, lane, wave_ln(xr, v_cnw, v_cnb, lane));       // ca_block.norm -> input of the query (mdiff_transformer.py:229)
                }
                st4(RES + 4 * lane, xr);
            } else if constexpr (WIN) {
                cl_flag_wait(FLG + 1, e2);
                cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::W2A{});
                cl_flag_wait(FLG + 2, e2);
                cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::W2B{});
            }
            __syncthreads(); DEN_DBG(0);

            if constexpr (Q) {
                // ================= G: ca_block.query, column-split by dims (waves < S / 16 own one tile each) -> X3 =================
                if constexpr (!WIN) cl_refills<WT, C, Q, G::U_C + C_INL>(ring, wave, voff, wg, bc, bn, skip, nskip, std::make_integer_sequence<int, G::TB - C_INL>{});   // slots of stage C
                {
                    f32x4 acc[1];
                    cl_zero<1>(acc);
                    const bool act = wave < G::S / 16;
                    cl_units<WT, C, Q, G::U_G, 1, 1, 0, 0, 0>(ring, xb, acc, act, wave, voff, wg, bc, bn, skip, nskip, std::make_integer_sequence<int, 1>{});
                    if (act && lane < 16) QS[wave * 16 + col] = cl_out<WT>(acc[0]) + v_caq_b[c * G::S + wave * 16 + col];
                }
                __syncthreads(); DEN_DBG(0);
                if (epi) {
                    // The query softmax runs over all 256 dims (one head), the key softmax over the N tokens per dim (mdiff_transformer.py:231-232).
                    // This CU holds S dims: local maximum m, e = exp(q - m), l = sum e, and per token t_n = sum_d e_d kc_n[d]; the cluster
                    // combines them like a split softmax: M = max m_c, w_c = exp(m_c - M), dot_n = sum_c t_cn w_c / sum_c l_c w_c.
                    const unsigned epoch = e3;
                    float m = -INFINITY;
#pragma unroll
                    for (int dd = 0; dd < G::S; dd += 64) { const int d = dd + lane; if (d < G::S) m = fmaxf(m, QS[d]); }
                    m = wave_max(m);
                    float lsum = 0.f, tn[DCL_MAX_N];
#pragma unroll
                    for (int n = 0; n < DCL_MAX_N; ++n) tn[n] = 0.f;
#pragma unroll
                    for (int dd = 0; dd < G::S; dd += 64) {
                        const int d = dd + lane;
                        if (d < G::S) {
                            const float e = fast_exp(QS[d] - m);
                            lsum += e;
                            float kr[DCL_MAX_N], kmx = -INFINITY, ks = 0.f;
#pragma unroll
                            for (int n = 0; n < DCL_MAX_N; ++n) if (n < N) { kr[n] = CT[n * 1024 + 512 + c * G::S + d]; kmx = fmaxf(kmx, kr[n]); }
#pragma unroll
                            for (int n = 0; n < DCL_MAX_N; ++n) if (n < N) { kr[n] = fast_exp(kr[n] - kmx); ks += kr[n]; }
                            const float rks = fast_rcp(ks);
#pragma unroll
                            for (int n = 0; n < DCL_MAX_N; ++n) if (n < N) tn[n] = fmaf(e, kr[n] * rks, tn[n]);
                        }
                    }
                    lsum = wave_sum(lsum);
#pragma unroll
                    for (int n = 0; n < DCL_MAX_N; ++n) tn[n] = wave_sum(tn[n]);
                    {
                        float pv = lane == 0 ? m : (lane == 1 ? lsum : 0.f);
#pragma unroll
                        for (int n = 0; n < DCL_MAX_N; ++n) pv = lane == 2 + n ? tn[n] : pv;
                        if (lane < 8) cl_store_granule(xg + G::G_X3 + c * 8 + lane, epoch, pv, local);
                    }
                    if constexpr (WIN) {
                        __builtin_amdgcn_sched_barrier(0);
                        cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::WXA{});
                        if (lane == 0) cl_flag_set(FLG + 1, e3);
                        __builtin_amdgcn_s_sleep(DCL_POLL_SLEEP);
                    }
                    const unsigned o3 = (unsigned)((G::G_X3 + (lane % C) * 8) * 8);
                    u32x4 g3[4];
                    unsigned spins = 0;
                    for (;;) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) g3[j] = __builtin_amdgcn_raw_buffer_load_b128(xr_, o3 + 16 * j, 0, 16);
                        unsigned ok = 1u;
#pragma unroll
                        for (int j = 0; j < 4; ++j) ok &= cl_tags_ok(g3[j], epoch);
                        if (__all(ok != 0u) || dead) break;
                        if (++spins > DCL_SPIN_LIMIT) { dead = true; if (lane == 0) atomicOr(ka.hdr, 8u); break; }
                    }
                    if constexpr (WIN) {
                        cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::WXB{});
                        if (lane == 0) cl_flag_set(FLG + 2, e3);
                    }
                    DEN_DBG(0);
                    // lane group of C publishers: [m, l, t_0 .. ] of publisher lane % C
                    const float mc = __uint_as_float(g3[0].x), lc = __uint_as_float(g3[0].z);
                    float M = mc;
                    if (C >= 2) M = fmaxf(M, dpp_f(M, 0));
                    if (C >= 4) M = fmaxf(M, dpp_f(M, 1));
                    if (C >= 8) M = fmaxf(M, dpp_f(M, 2));
                    const float wc = fast_exp(mc - M);
                    float Lw = lc * wc;
                    if (C >= 2) Lw += dpp_f(Lw, 0);
                    if (C >= 4) Lw += dpp_f(Lw, 1);
                    if (C >= 8) Lw += dpp_f(Lw, 2);
                    const float rL = fast_rcp(Lw);
                    float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int n = 0; n < DCL_MAX_N; ++n) {
                        if (n < N) {
                            float t = __uint_as_float((n & 1) ? g3[1 + (n >> 1)].z : g3[1 + (n >> 1)].x) * wc;
                            if (C >= 2) t += dpp_f(t, 0);
                            if (C >= 4) t += dpp_f(t, 1);
                            if (C >= 8) t += dpp_f(t, 2);
                            y = f4_fma(t * rL, ld4(CT + n * 1024 + 768 + 4 * lane), y);            // (q k^T) v  (:236-237)
                        }
                    }
                    // StylizationBlock (mdiff_transformer.py:152-163): SiLU(LN(y) (1 + scale) + shift) -> proj_out.out_layers
                    const float4 hh = f4_adaln(wave_ln(y, v_csnw, v_csnb, lane), ld4(TTS + 512 + 4 * lane), ld4(TTS + 768 + 4 * lane));
                    put_x<WT, 1>(XB, 0, 0, lane, f4_silu(hh));
                } else if constexpr (WIN) {
                    cl_flag_wait(FLG + 1, e3);
                    cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::WXA{});
                    cl_flag_wait(FLG + 2, e3);
                    cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::WXB{});
                }
                __syncthreads(); DEN_DBG(0);
                // ================= H: ca_block.proj_out.out_layers + residual (replicated) =================
                if constexpr (!WIN) cl_refills<WT, C, Q, G::U_G>(ring, wave, voff, wg, bc, bn, skip, nskip, std::make_integer_sequence<int, 1>{});                    // slot of stage G
                nxt.load(2, wave, lane, vp, Ln, tt_next, ln, A, b, c, ca_next, ca_R);
                {
                    f32x4 acc[2];
                    cl_zero<2>(acc);
                    cl_units<WT, C, Q, G::U_H, 2, 2, 0, 0, (WIN ? 0 : 2)>(ring, xb, acc, true, wave, voff, wg, bc, bn, skip, nskip, std::make_integer_sequence<int, 2>{});
                    if (lane < 32) {
                        const int n = (2 * wave + (lane >> 4)) * 16 + col;
                        const float x3 = RES[n] + ((lane & 16) ? cl_out<WT>(acc[1]) : cl_out<WT>(acc[0])) + v_cao_b[n];
                        RES[n] = x3;
                        cl_put1<WT>(XA, n, x3);
                    }
                }
                nxt.store(lane, STG + (cur ^ 1) * stg_sz);
                __syncthreads(); DEN_DBG(0);
            }

            // ================= D: ffn.linear1 + GELU (replicated) =================
            if constexpr (Q) nxt.load(3, wave, lane, vp, Ln, tt_next, ln, A, b, c, ca_next, ca_R);
            if constexpr (!Q && !WIN) cl_refills<WT, C, Q, G::U_C + C_INL>(ring, wave, voff, wg, bc, bn, skip, nskip, std::make_integer_sequence<int, G::TB - C_INL>{});       // slots of stage C
            if constexpr (GRP) {      // (G1 computes; this group requests the next layer's A0)
                clg_issue<0>(gr, gvoff, wg, bn + (unsigned)G::U_A * W::UNIT_BYTES, true, nskip || w4 < 2);
            } else {
                f32x4 acc[1];
                cl_zero<1>(acc);
                cl_units<WT, C, Q, G::U_D, 1, 1, 0, 0, (WIN ? 0 : 1)>(ring, xa, acc, true, wave, voff, wg, bc, bn, skip, nskip, std::make_integer_sequence<int, 1>{});
                if (lane < 16) {
                    const int j = wave * 16 + col;
                    cl_put1<WT>(XH, j, fast_gelu(cl_out<WT>(acc[0]) + v_f1b[j]));
                }
            }
            if constexpr (Q) nxt.store(lane, STG + (cur ^ 1) * stg_sz);
            __syncthreads(); DEN_DBG(0);
            // ================= E: ffn.linear2 -> LayerNorm, AdaLN, SiLU (replicated) =================
            if constexpr (GRP) {
                f32x4 acc[2][2];
                uint4 fr[4];
                clg_frags<4>(fr, xh);
                __builtin_amdgcn_sched_barrier(0);
                cl_zero<2>(acc[0]); cl_zero<2>(acc[1]);
                clg_consume<WT, 2, 4, 0>(gr.r[1], fr, acc);
                cl_pin<2>(acc[0]); cl_pin<2>(acc[1]);
                PART[(2 * (w4 + 4 * (lane >> 5)) + ((lane >> 4) & 1)) * 16 + col] = clg_out<WT, 2>(acc, lane);
            } else {
                f32x4 acc[2];
                cl_zero<2>(acc);
                cl_units<WT, C, Q, G::U_E, 1, 2, 0, 0, (WIN ? 0 : 1)>(ring, xh, acc, true, wave, voff, wg, bc, bn, skip, nskip, std::make_integer_sequence<int, 1>{});
                if (lane < 32) PART[(2 * wave + (lane >> 4)) * 16 + col] = (lane & 16) ? cl_out<WT>(acc[1]) : cl_out<WT>(acc[0]);
            }
            __syncthreads(); DEN_DBG(0);
            if (epi) {
                if constexpr (WIN) {
                    cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::W3{});
                    if (lane == 0) cl_flag_set(FLG + 3, e2);
                }
                const float4 y2 = f4_add(ld4(PART + 4 * lane), ld4(v_f2b + 4 * lane));
                const float4 hh = f4_adaln(wave_ln(y2, v_fsnw, v_fsnb, lane), ld4(TFS + 4 * lane), ld4(TFS + 256 + 4 * lane));
                put_x<WT, 1>(XB, 0, 0, lane, f4_silu(hh));
            } else if constexpr (WIN) {
                cl_flag_wait(FLG + 3, e2);
                cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::W3{});
            }
            __syncthreads(); DEN_DBG(0);
            // ================= F: ffn.proj_out.out_layers + residual (replicated); writes the next layer's input =================
            if constexpr (Q) nxt.load(4, wave, lane, vp, Ln, tt_next, ln, A, b, c, ca_next, ca_R);
            if constexpr (WIN) __builtin_amdgcn_sched_barrier(0);   // (the fence of a window that requests nothing any more; without it stage F's first fragment reads move up)
            if constexpr (GRP) {      // (G1 computes; this group requests the next layer's A1, the skip half -- ONE request site for all four waves:
                                      //  requested in the ffn-epilogue window, before / behind the release, the slot is kept twice and copied)
                clg_issue<1>(gr, gvoff, wg, bn + (unsigned)G::U_AS * W::UNIT_BYTES, nskip, nskip);
            } else {
                f32x4 acc[2];
                cl_zero<2>(acc);
                cl_units<WT, C, Q, G::U_F, 2, 2, 0, 0, (WIN ? 0 : 2)>(ring, xb, acc, true, wave, voff, wg, bc, bn, skip, nskip, std::make_integer_sequence<int, 2>{});
                if constexpr (WIN) cl_issue_seq<WT, C, Q>(ring, wave, voff, wg, bc, bn, skip, nskip, typename SCH::AF{});
                if (lane < 32) {
                    const int n = (2 * wave + (lane >> 4)) * 16 + col;
                    const float xn = RES[n] + ((lane & 16) ? cl_out<WT>(acc[1]) : cl_out<WT>(acc[0])) + v_fo_b[n];
                    RES[n] = xn;
                    cl_put1<WT>(XA, n, xn);
                    if (l < 2) cl_put1<WT>(SKF + 512 * l, n, xn);                      // xs.append(x) (cross_attention.py:70-72)
                }
            }
            if constexpr (Q) nxt.store(lane, STG + (cur ^ 1) * stg_sz);
            // (phantom units that pad the layer program are never consumed: the re-fills they would trigger go out here)
            if constexpr (!WIN) cl_refills<WT, C, Q, G::NU_REAL>(ring, wave, voff, wg, bc, bn, skip, nskip, std::make_integer_sequence<int, G::NU - G::NU_REAL>{});
            __syncthreads(); DEN_DBG(0);
            if (l + 1 < SEEME_DEN_NL) {
                if (epi && !nskip) xr = ld4(RES + 4 * lane);                          // residual of the next layer's attention
            } else {
                // ---- stack norm -> model output (cross_attention.py:82-83), scheduler.step (mld.py:495-497)
                if (epi) {
                    float4 e = wave_ln(ld4(RES + 4 * lane), CONSTV + 256, CONSTV + 512, lane);
                    if (A.sched == SEEME_SCHED_NONE) {
                        st4(KEEP + 4 * lane, e);
                    } else {
                        // two wave groups: coefficients and noise row are in LDS since this step's X1 windows (ClRowG)
                        const SchedCoef k = GRP ? sched_coef_lds(COEF) : sched_coef_row(A.coef, step);
                        float4 nz = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (A.noise != nullptr) nz = ld4(GRP ? NZ + 4 * lane : sched_noise_row(A.noise, A.B, step, b, lane));
                        const float4 nl = sched_step(ld4(KEEP + 4 * lane), e, nz, k);
                        st4(KEEP + 4 * lane, nl);
                        xr = f4_add(nl, ld4(CONSTV + 4 * lane));
                        put_x<WT, 1>(XA, 0, 0, lane, xr);
                        st4(RES + 4 * lane, xr);
                    }
                }
                __syncthreads(); DEN_DBG(0);
            }
            cur ^= 1;
        }
        row = GRP ? row_nx : row_next;
    }
    DEN_DBG(3);
    if (epi && c == 0) st4(A.out + (size_t)b * 256 + 4 * lane, ld4(KEEP + 4 * lane));
    if constexpr (GRP) {
#pragma unroll
        for (int s = 0; s < 2; ++s) asm volatile("" ::"v"(gr.r[s][0][0].x));
    } else {
#pragma unroll
        for (int s = 0; s < W::RU; ++s) asm volatile("" ::"v"(ring.r[s][0].x));
    }
}

template <int C>
static size_t cl_lds_bytes(int N, bool q, bool grp) {
    typedef ClG<C> G;
    const int stg = q ? 2 * (VP_LAYER + STG_TT + N * 1024) : ClRes<C>::FLOATS;    // (one condition token: resident block + changing rows)
    const int sch = grp ? 12 + 256 : 0;                                            // (two wave groups: COEF | NZ, the same for every plan)
    return (size_t)(768 + 256 + stg + 512 + 512 + 2 * (G::NB > 128 ? G::NB : 128) + 1024 + 2 * G::S + 256 + 256 + 4 + sch) * sizeof(float);
}

extern "C" size_t seeme_den_cluster_xchg_bytes(int B, int C) {       // (the several-token layout: the larger of the two)
    const size_t per = C == 8 ? ClG<8, true>::G_TOTAL : (C == 4 ? ClG<4, true>::G_TOTAL : ClG<2, true>::G_TOTAL);
    const size_t clusters = (size_t)(B + 7) / 8 * 8;
    return DCL_HDR_BYTES + clusters * per * 8;
}
// query = 0: one condition token (tabulated ca term); 1: several (the ca_block's query and proj_out stages are units of the image).
// out[0] = units per (layer, CU) incl. phantom padding, [1] = bytes per unit, [2] = image bytes, [3] = wave-loads per unit, [4] = k per wave-load,
// [5..11] = first unit of A (x half), A (skip half), B, C, D, E, F, [12] = first unit of G (ca query; -1 without), [13] = of H (ca proj_out)
extern "C" int seeme_den_cluster_layout(int C, int wdtype, int query, int64_t* out, int cap) {
    if (cap < 14) return seeme_fail("den_cluster_layout: output too small");
    if (C != 2 && C != 4 && C != 8) return seeme_fail("den_cluster_layout: C must be 2, 4 or 8");
    const int TA = 256 / C / 32, TB = 8 / C;
    const int u_c = 2 * TA + TB, u_g = u_c + TB, u_d = query ? u_g + 3 : u_g;
    const int64_t NU = (u_d + 4 + 3) / 4 * 4, UL = wdtype == 0 ? 16 : 8, UB = 8 * UL * 1024;
    out[0] = NU; out[1] = UB; out[2] = (int64_t)SEEME_DEN_NL * C * NU * UB; out[3] = UL; out[4] = 256 / UL;
    out[5] = 0; out[6] = TA; out[7] = 2 * TA; out[8] = u_c; out[9] = u_d; out[10] = u_d + 1; out[11] = u_d + 2;
    out[12] = query ? u_g : -1; out[13] = query ? u_g + 1 : -1;
    return 0;
}

template <typename WT, int C, bool Q>
static int launch_den_cluster(const ClArgs& ka0, hipStream_t st, bool zeroed) {
    ClArgs ka = ka0;
    ka.clusters = (ka.s.B + 7) / 8 * 8;
    const int grid = ka.clusters * C;
    // co-residency of every workgroup is what the in-launch exchanges rest on: one workgroup per CU of THIS device (a partitioned or
    // CU-masked device has fewer than 256)
    int dev = 0, cus = 0;
    SEEME_HIP(hipGetDevice(&dev));
    SEEME_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (grid > cus || grid > 256) return seeme_fail("denoiser_sample_cluster: B x C exceeds one workgroup per CU of this device");
    const size_t lds = cl_lds_bytes<C>(Q ? ka.s.N : 1, Q, ClGrp<WT, C, Q>::ON);
    if (lds > 160 * 1024 || lds <= 80 * 1024) return seeme_fail("denoiser_sample_cluster: LDS footprint must force one workgroup per CU");
    SEEME_HIP(hipFuncSetAttribute((const void*)k_den_cluster<WT, C, Q>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // granules and header are zeroed before EVERY launch (tags of an earlier launch must never match)
    if (!zeroed) SEEME_HIP(hipMemsetAsync(ka.hdr, 0, seeme_den_cluster_xchg_bytes(ka.s.B, C), st));
    hipLaunchKernelGGL((k_den_cluster<WT, C, Q>), dim3(grid), dim3(DEN_THREADS), lds, st, ka);
    return seeme_check_launch("k_den_cluster");
}
template <typename WT>
static int launch_den_cluster_c(const ClArgs& ka, int C, bool q, hipStream_t st, bool zeroed) {
    if (C == 8) return q ? launch_den_cluster<WT, 8, true>(ka, st, zeroed) : launch_den_cluster<WT, 8, false>(ka, st, zeroed);
    if (C == 4) return q ? launch_den_cluster<WT, 4, true>(ka, st, zeroed) : launch_den_cluster<WT, 4, false>(ka, st, zeroed);
    if (C == 2) return q ? launch_den_cluster<WT, 2, true>(ka, st, zeroed) : launch_den_cluster<WT, 2, false>(ka, st, zeroed);
    return seeme_fail("denoiser_sample_cluster: C must be 2, 4 or 8");
}

static int den_cluster_ms_dispatch(const SeemeDenoiserWeights* w, const SeemeDenCluster* cl, const SeemeSampleArgs* a, ClArgs& ka, hipStream_t st, bool zeroed);   // den_cluster_ms.inc.hip

extern "C" int seeme_denoiser_sample_cluster(const SeemeDenoiserWeights* w, const SeemeDenCluster* cl, const SeemeSampleArgs* a, void* stream) {
    if (int rc = den_check_sample_args("denoiser_sample_cluster", a)) return rc;
    if (a->N < 1 || a->N > DCL_MAX_N) return seeme_fail("denoiser_sample_cluster: 1 or 2 condition tokens");
    const bool q = a->N > 1;
    if (!q && (a->catab == nullptr || a->force_query)) return seeme_fail("denoiser_sample_cluster: one condition token needs its ca table");
    if (q != (cl->query != 0)) return seeme_fail("denoiser_sample_cluster: the weight image was packed for the other ca_block variant (SeemeDenCluster.query)");
    if (w->nhead != 1 || !w->sa_fold) return seeme_fail("denoiser_sample_cluster: one attention head (folded out_proj)");
    if (a->cfg || a->save != nullptr) return seeme_fail("denoiser_sample_cluster: no CFG pair, no training forward");
    if (w->ff_sa != FF_SA || w->ff != FF_D) return seeme_fail("denoiser_sample_cluster: built for sa ff 1024 / ffn_dim 128");
    const bool ms = cl->samples > 1;
    if (cl->xchg == nullptr || (!ms && cl->xchg_bytes < seeme_den_cluster_xchg_bytes(a->B, cl->C))) return seeme_fail("denoiser_sample_cluster: exchange buffer too small");
    if (((uintptr_t)cl->xchg & 15) != 0) return seeme_fail("denoiser_sample_cluster: exchange buffer must be 16-byte aligned");
    int64_t lo[14];
    int rc = seeme_den_cluster_layout(cl->C, cl->wdtype, q ? 1 : 0, lo, 14);
    if (rc) return rc;
    ClArgs ka;
    ka.wgc = cl->wgc; ka.wgc_bytes = (unsigned)lo[2]; ka.vp = cl->vpc;
    ka.lay = seeme_make_den_layout(FF_SA, FF_D);
    ka.s = *a;
    ka.hdr = (unsigned*)cl->xchg;
    ka.xg = (unsigned long long*)((char*)cl->xchg + DCL_HDR_BYTES);
    ka.placement = cl->placement; ka.flags = cl->flags; ka.clusters = 0; ka.spc = 1;
    hipStream_t st = (hipStream_t)stream;
    const bool zeroed = cl->xchg_zeroed != 0;     // the caller zeroed granules and header on this stream (seeme_denoiser_tables1)
    if (ms) return den_cluster_ms_dispatch(w, cl, a, ka, st, zeroed);
    if (cl->wdtype == 0) return launch_den_cluster_c<WF32>(ka, cl->C, q, st, zeroed);
    if (cl->wdtype == 1) return launch_den_cluster_c<WBF16>(ka, cl->C, q, st, zeroed);
    if (cl->wdtype == 2) return launch_den_cluster_c<WF16>(ka, cl->C, q, st, zeroed);
    return seeme_fail("denoiser_sample_cluster: wdtype must be 0 (fp32), 1 (bf16) or 2 (fp16)");
}
