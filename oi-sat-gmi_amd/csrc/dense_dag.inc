// Task-graph Cholesky: the whole factorization of one system -- or of a month's fifty -- as ONE persistent launch.
// The device half.  (Included by dense_dag.hip alone, inside its anonymous namespace, behind dense_tile.inc, dense_kloop.inc (LDS-DMA
// K-loop), dense_diag.inc (diagonal-block waves), dense_trsv.inc (sweep rows) and dense_solve_dev.inc (residual, increment).  The launch's
// types are in dense_internal.h, dag_launch in dense_dag.hip, the plan and the ticket order, host code, in dense_dag_plan.hip.)
//
// Why: for 4,000-18,000 observations the recursive schedule is a chain of ~3 dependent launches per diagonal block (diagonal
// block 19 us on ONE workgroup, panel 9 us, rank-128 update 12 us: 3.4 of the 8 ms of a 10,000-observation analysis) next to
// ~100 launches that are too small to fill 256 CUs.  Here the dependencies are per TILE instead of per launch:
//   * LEFT-LOOKING tile tasks.  Task T(i, j), i >= j + 2, owns tile (i, j): it accumulates  sum_k L(i,k) L(j,k)^T  over
//     k = 0 .. j-1 in its MFMA accumulators -- one long K-loop, consumed block column by block column as the two row panels
//     become final -- then forms  (S(i,j) - acc) T_j^T  and publishes L(i,j).  No read-modify-write of C between updates, no
//     launch boundaries; a tile's K-loop runs ahead as far as its inputs exist and then waits for the newest block column.
//   * one CHAIN workgroup per system walks the diagonal: diagonal block j (the register-resident potrf_diag3 waves), panel
//     tile (j+1, j), rank-128 update of (j+1,j+1) with that tile straight from LDS.  The older updates of (j,j) and (j+1,j)
//     come from bulk tasks PRE(j) / SUB(j), which leave the updated tile in S.  The chains of the largest systems get a CU
//     to themselves (CU census at the start of the launch).
//   * progress words per system (agent scope): diagdone, rowfin[r] = number of final blocks L(r, 0 .. rowfin-1) of block row r
//     (they become final in order), pre[j], sub[j].  Produced tiles are stored write-through (`sc1`), the storing waves drain
//     vmcnt, the workgroup meets at a barrier and one lane publishes; a consumer polls with agent-scope loads, runs one agent
//     acquire, meets at a barrier and reads with plain loads / LDS-DMA; producers also drop the L1 lines that would be stale
//     ("L1 hygiene" below), so the acquire is a second line of defence.
//   * tasks are drawn by TICKET from one list in an order that is topological for the whole graph (chain steps included):
//     systems in waves, a wave's systems column-major and interleaved by the fraction of their columns.  A task only waits for lower tickets
//     and for the chains of its wave.  A chain, though, waits for HIGHER tickets (sub(j) / pre(j+1) come from bulk tasks), so
//     the launch drains only if, next to a wave's chains, at least one more workgroup is resident to draw them: the host
//     refuses a launch whose largest wave has more chains than a quarter of the resident workgroups (dag_launch) and the
//     caller falls back to the lock-step recursion.  Every spin is bounded; a time-out raises the launch's error word,
//     which every other spin reads, and is counted in the handle's task-graph time-out word (oisat_solve_status_ex).

// thread 0: wait until *p >= v (agent-scope polls); false = time-out or another workgroup's error
__device__ __forceinline__ bool dag_wait_ge(const int* p, int v, DagCtl* ctl, unsigned spin_max) {
    unsigned spins = 0;
    while (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) {
        __builtin_amdgcn_s_sleep(2);
        if ((++spins & 255u) == 0u &&
            (spins > spin_max || __hip_atomic_load(&ctl->error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
            __hip_atomic_store(&ctl->error, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
    }
    return true;
}

// L1 hygiene.  A CU's vector L1 is never refreshed by other CUs' stores, so a line that holds a tile's NOT-YET-FINAL content must
// not survive in a CU's L1 until some workgroup of that CU reads the final tile.  Lines with pre-final content get into an
// L1 three ways: (a) `sc1` loads of a C tile (read-modify-write): they force a miss, but the fetched line stays; (b) this
// workgroup's own stores of an intermediate result (X = S(i,j) - acc of a tile task, the updated tile SUB(j) leaves): write-
// through, and the local line is updated; (c) the LDS-DMA read of such an intermediate tile as the operand of the panel
// product (tile task: its own X; chain: the tile SUB(j) left).  Whoever does any of these to a tile that will later be read
// as an OPERAND drops its CU's L1 once (one buffer_inv, completed by a vmcnt(0) in front of its publish) after the LAST
// WAVE's last such access and before it publishes: the tile task and the chain behind the final barrier of the panel
// product's K-segment, SUB(j) / PRE(j) behind a barrier that follows their epilogue.  Every operand read is then a first touch of final data on its CU, and consumers
// need no acquire: a poll, a barrier, plain loads / LDS-DMA.  Across XCDs: a tile is only ever read by the workgroup that is
// about to rewrite it until it is final, and write-through stores drop the line from that XCD's L2, so no L2 holds an old copy.
// (Found the hard way: without the drop in SUB(j) -- (a) was thought to leave nothing behind -- tools/dag_stress.py, three
// factorizations on three streams under bursty memory traffic, saw one wrong factor in ~5,000: a tile task that landed on the
// CU where SUB(j) had run read L(j+1,j) as SUB(j) had left it.  Both lines of defence -- the producers' drops and the consumers'
// acquires -- are unconditional in the product.)
// The shadow (dag_shadow_store) needs nothing more: a shadow tile is written exactly ONCE per launch, write-through, with its
// final content, in front of the publish of the rowfin word that announces the fp32 tile, and nobody reads it before that
// word -- there is no pre-final content of it that an L1 or another XCD's L2 could hold; what a previous launch left in a
// cache is gone at the launch boundary, as for S itself.
__device__ __forceinline__ void dag_drop_l1() { asm volatile("buffer_inv sc1" ::: "memory"); }

// consumer side, whole workgroup: thread 0 has polled (ok = its verdict)
__device__ __forceinline__ bool dag_join(bool ok_thread0, int* s_flag) {
    if (threadIdx.x == 0) {
        *s_flag = ok_thread0 ? 1 : 0;
        // one agent acquire by the polling lane, inside the barrier the workgroup meets at anyway (no measurable cost: 3.66 vs
        // 3.67 ms at 10,000 observations, 301.2 vs 301.6 ms at 50,000).  The producers' L1 drops make it redundant; both stay.
        asm volatile("buffer_inv sc1\n\ts_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    return *s_flag != 0;
}

// producer side, whole workgroup: every storing wave drains its (write-through) stores, barrier, one lane publishes
__device__ __forceinline__ void dag_publish(int* p, int v) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The same K-segment on the bf16 matrix pipe -- the FAR stretch of a bulk task's K-loop (kfar, "Far stretch" at
// dag_task_order): over the SAME fp32 LDS image and the same LDS-DMA fill as dag_seg, nothing changes in memory.  A K-step
// of 32 is two k-chunks of 16.  v_mfma_f32_32x32x16_bf16 takes A[row lane & 31][k = 8 (lane >> 5) + e], e = 0 .. 7, from
// each lane -- and B likewise --, so a lane reads the 8 consecutive floats 16 c + 8 fh .. + 7 of its operand row: the logical
// 16-byte chunks 4 c + 2 fh and + 1 through the image's XOR swizzle (over the 32 rows of a half-wave the same bank pattern
// as dag_seg's fragment reads), rounds them to nearest even with v_cvt_pk_bf16_f32 and issues the four MFMAs of its 64 x 64
// quadrant into the same accumulators (the C/D layout does not depend on the operand type).  1/16 of dag_seg's MFMA cycles
// per K-step, the same LDS reads; what bounds a far K-step is the landing of its LDS-DMA (one step of look-ahead), and a
// workgroup that waits for it leaves the matrix pipe to its CU-mate.
typedef __attribute__((ext_vector_type(8))) __bf16 dag_bf16x8;
typedef __attribute__((ext_vector_type(4))) unsigned dag_u32x4;
__device__ __forceinline__ unsigned dag_pk_bf16(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
__device__ __forceinline__ dag_bf16x8 dag_pack8(const float4& a, const float4& b) {
    const dag_u32x4 u = {dag_pk_bf16(a.x, a.y), dag_pk_bf16(a.z, a.w), dag_pk_bf16(b.x, b.y), dag_pk_bf16(b.z, b.w)};
    return __builtin_bit_cast(dag_bf16x8, u);
}

// ... and as SPLIT bf16 products -- the MIDDLE stretch of a bulk task's K-loop (kmid, "Middle stretch" at dag_task_order):
// the far stretch's LDS image, LDS-DMA fill, barriers and fragment reads, but every operand fragment a becomes
// two bf16 fragments, hi = bf16(a) (round to nearest even, the far stretch's own rounding) and lo = bf16(a - float(hi)) --
// a - float(hi) is exact in fp32 -- and a product a b^T becomes lo hi^T + hi lo^T + hi hi^T: relative error ~2^-16 per term
// (the dropped lo lo^T and the rounding of lo) where the far stretch has 2^-8.  Twelve MFMAs per k-chunk into the same four
// accumulators, in ONE order: a_lo b_hi^T of the quadrants 00, 01, 10, 11, then a_hi b_lo^T of the four, then a_hi b_hi^T of
// the four -- every accumulator takes its small terms first, and no MFMA waits for the one issued in front of it.  3/16 of
// dag_seg's MFMA cycles per K-step; the split is VALU work, ~3 instructions per operand element (unpack, subtract, pack),
// operand by operand so that the raw fp32 fragment of one operand is dead before the next is split.
__device__ __forceinline__ unsigned dag_pk_bf16_lo(float x, float y, unsigned hi /* dag_pk_bf16(x, y) */) {
    return dag_pk_bf16(x - __builtin_bit_cast(float, hi << 16), y - __builtin_bit_cast(float, hi & 0xffff0000u));
}
__device__ __forceinline__ void dag_split8(const float4& a, const float4& b, dag_bf16x8& hi, dag_bf16x8& lo) {
    const dag_u32x4 h = {dag_pk_bf16(a.x, a.y), dag_pk_bf16(a.z, a.w), dag_pk_bf16(b.x, b.y), dag_pk_bf16(b.z, b.w)};
    const dag_u32x4 l = {dag_pk_bf16_lo(a.x, a.y, h.x), dag_pk_bf16_lo(a.z, a.w, h.y), dag_pk_bf16_lo(b.x, b.y, h.z), dag_pk_bf16_lo(b.z, b.w, h.w)};
    hi = __builtin_bit_cast(dag_bf16x8, h);
    lo = __builtin_bit_cast(dag_bf16x8, l);
}

// ---- Shadow: the bf16 images of the final tiles, made once -----------------------------------------------------------------
// A finished tile L(r,k) is an operand of up to a band's width of later tasks, and every one of them rounded it (far) or
// split it (middle) again in its K-loop: 96 VALU instructions per lane and k-chunk in front of the middle stretch's MFMAs,
// and four bytes fetched per element where the far stretch needs two.  hi = bf16(a) and lo = bf16(a - float(hi)) are pure
// functions of the final tile, so the task that stores a final off-diagonal tile stores them too (dag_shadow_store) and the
// two stretches DMA them (dag_seg_sh): the same operand bits into the same MFMAs in the same order as the in-loop
// conversions (dag_seg_bf16 / dag_seg_bf16x2) -- the factor does not change by a bit.
// Layout of a shadow tile (kShTile = 64 KiB, tiles of a block row consecutive in k; DagSys::shadow): two PLANES, hi then lo,
// each [group g = 0 .. 7][row 0 .. 127][16 columns 16 g .. 16 g + 15] in bf16 -- a group is 4 KiB contiguous, 32 bytes per
// row.  Only LDS-DMA reads it, in UNITS of 16 KiB of LDS, [A | B][128 rows x 64 bytes], whose source is contiguous per operand:
//   * a FAR unit is 32 columns of the hi plane, two consecutive groups (8 KiB contiguous): the image row is 4 chunks of 8
//     columns, k-chunk c = 0, 1 of a lane is the logical chunk 2 c + fh -- one ds_read_b128 where the conversion has two and
//     four packs, and two bytes fetched per element where it has four;
//   * a MIDDLE unit is 16 columns: group g of the hi plane (logical chunks 0, 1 of the image row) | group g of the lo plane
//     (chunks 2, 3); its one k-chunk is the chunks fh (hi) and 2 + fh (lo).
// A tile is 4 far units or 8 middle ones.  The LDS side of an LDS-DMA is lane-linear, so the swizzle is on the SOURCE: lane l
// of a piece of 16 rows lands at physical chunk l & 3 of row l >> 2 and fetches the logical chunk (l & 3) ^ ((row >> 2) & 3);
// a fragment read takes logical chunk q of its row at physical chunk q ^ ((row >> 2) & 3).  Checked by enumeration against
// the lane groups a ds_read_b128 is served in ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32; bank = (byte / 4)
// mod 64): the 16 rows of a group are four rows of each residue mod 4 -- which picks the 64-byte quarter of the 256-byte
// bank row -- and their (row >> 2) & 3 are {0, 3, 1, 2} / {1, 2, 0, 3}, four different chunks of that quarter: every group
// covers the 64 banks exactly once, for every q.  (row & 3, dag_seg's rule for 128-byte rows scaled down, would be 4-way.)
// No cache line holds parts of two tiles.
// Tried and not kept: the images BEHIND the publish of rowfin, announced by a progress word of their own that the shadow
// segments poll instead, with the chain's images converted from its LDS image under the rank-128 update's MFMAs.  The chain's
// panel step went back from 15.3 to 12.8 us, but its rank-128 update rose from 7.8 to 10.3 us and its diagonal block from 22.9
// to 24.8 us: the headline step was the same to 0.1 ms, for a fourth progress array and a second writer.
// (kShTile, kShPlane, kShGroup -- bytes of a shadow tile, of a plane, of a 16-column group of a plane -- are in dense_internal.h:
// the host sizes the shadow and reads a tile back with them, dense_chol.hip)
constexpr int kShUnit = 16384;                                  // bytes of a unit in LDS; the workgroup's image holds four
// The segment's RING: kShRing stages of 4 / kShRing units each, kShAhead stages' DMAs in flight while one is consumed.
// 2 | 1: one 32 KiB stage ahead, every wait a vmcnt(0) -- the default.  4 | 3: three half-size stages ahead, counted waits;
// 4 | 2: the shallower pipeline of the same stages.  All three were measured from these two constants (4 | 2: kShAhead = 2; profiles/EXPERIMENTS.md,
// "A ring of four stages"): at lead 0.2 4 | 3 is 0.36 ms of the headline step ahead of 2 | 1 and missed the bar set for it; at the
// lead that ships the two measure the same.
constexpr int kShRing = 2;
constexpr int kShAhead = kShRing - 1;
constexpr int kShStageUnits = 4 / kShRing;
constexpr int kShStagePieces = 4 * kShStageUnits;               // LDS-DMA instructions per wave and stage: 2 per operand and unit
static_assert((kShRing == 2 || kShRing == 4) && kShAhead >= 1 && kShAhead < kShRing, "a stage is refilled one barrier behind its last read");
static_assert(kShStagePieces * kShAhead <= 63, "vmcnt is six bits");
// lane's DMA source inside the shadow tile at `tile`: row wid*32 + (lane >> 2) of the tile's first unit, far | middle (SPLIT)
template <bool SPLIT>
__device__ __forceinline__ const char* dag_sh_src(const char* tile, const DagLane& L) {
    const int q = (L.lane & 3) ^ ((L.lane >> 4) & 3);           // (the pieces start at multiples of 16 rows: (row >> 2) & 3 = (lane >> 4) & 3)
    return tile + (q >> 1) * (SPLIT ? kShPlane : kShGroup) + (L.wid * 32 + (L.lane >> 2)) * 32 + (q & 1) * 16;
}
// LDS-DMA of one unit into unit slot `us` of the image: wave `wid` brings rows wid*32 + 16 i .. + 15 (i = 0, 1) of each operand,
// one KiB per instruction.  a / b: dag_sh_src of the unit.
__device__ __forceinline__ void dag_sh_dma(float* __restrict__ lds, int us, const DagLane& L, const char* a, const char* b) {
    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        __builtin_amdgcn_global_load_lds((gptr_t)(a + 512 * i), (lptr_t)(lds + us * (kShUnit / 4) + (L.wid * 32 + 16 * i) * 16), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gptr_t)(b + 512 * i), (lptr_t)(lds + us * (kShUnit / 4) + kShUnit / 8 + (L.wid * 32 + 16 * i) * 16), 16, 0, 0);
    }
}
// The fragment reads are written out as instructions.  Left to the compiler, every ds_read behind an LDS-DMA that it cannot
// prove disjoint gets an s_waitcnt vmcnt(0) in front of it -- the whole ring would drain at the first read of every stage
// (it did so in the two-buffer loop this replaced: its look-ahead never overlapped anything).  The compiler then no longer
// counts these reads either: dag_lds_wait retires them, and takes the fragments as operands so that nothing that uses
// them moves in front of it.  What nothing enforces: to the compiler a fragment is complete at the read's asm statement, so a
// register copy or a spill of it placed between the read and its wait would move stale data.  The generated gfx950 code has
// reads, lgkmcnt, MFMAs and no move in between (0 spilled VGPRs); at a compiler upgrade the bit-equality tests
// (tests/test_gpu_seg_pipeline.py, test_gpu_factor_shadow.py) are the guard, and the .s is worth a look.
template <int OFF>
__device__ __forceinline__ dag_u32x4 dag_lds_rd(unsigned addr) {
    dag_u32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
template <int N>
__device__ __forceinline__ void dag_lds_wait(dag_u32x4& a, dag_u32x4& b, dag_u32x4& c, dag_u32x4& d) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N) : "memory");
}
__device__ __forceinline__ void dag_lds_wait_all(dag_u32x4& a, dag_u32x4& b, dag_u32x4& c, dag_u32x4& d, dag_u32x4& e, dag_u32x4& f, dag_u32x4& g,
                                                 dag_u32x4& h) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h) : : "memory");
}
template <int N>
__device__ __forceinline__ void dag_vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// the workgroup barrier of the ring: LDS traffic only -- __syncthreads() would drain the DMAs in flight
__device__ __forceinline__ void dag_ring_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}
template <int N> struct DagInt { static constexpr int value = N; };

// One K-segment over the shadow, nkb K-blocks (tiles) long: SPLIT = the middle stretch's split products (else the far
// stretch's single ones).  Ad / Bd: dag_sh_src<SPLIT> of the segment's first tile of each operand row.  The same operand bits
// into the same MFMAs in the same order as dag_seg_bf16 / dag_seg_bf16x2: k-chunk by k-chunk, the twelve MFMAs of a split
// k-chunk in dag_seg_bf16x2's order.
// INVARIANT: a tile is 4 far or 8 middle units, so a segment is a whole number of turns of the ring -- it starts and ends on
// ring slot 0, the kShAhead stages of the prologue always exist, and the loop body is half a turn -- 32 KiB of the image, whose
// slots differ from a constant by the turn's half (the code holds every MFMA as often as the loop it replaced).
// Phase s (stage s is in LDS and every wave is past the barrier behind the wait that retired it): issue stage s + kShAhead
// into the slot whose last reads were retired in front of the previous barrier; read and consume stage s; wait until at most
// kShAhead - 1 stages are in flight, i.e. this wave's pieces of stage s + 1 have landed; barrier.  The last stages drain
// with smaller counts, the last wait is vmcnt(0): on return everything has landed, every read is back and every wave is
// past a barrier, as after dag_seg.  On entry no wave reads or fills the image and this wave has no load in flight whose
// result the compiler still waits for (callers: a join or a segment's last barrier is behind every wave).
#define DAG_MFMA4_BF16(A0, A1, B0, B1)                                                          \
    acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(DAG_BF(A0), DAG_BF(B0), acc00, 0, 0, 0);    \
    acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(DAG_BF(A0), DAG_BF(B1), acc01, 0, 0, 0);    \
    acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(DAG_BF(A1), DAG_BF(B0), acc10, 0, 0, 0);    \
    acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(DAG_BF(A1), DAG_BF(B1), acc11, 0, 0, 0);
#define DAG_BF(X) __builtin_bit_cast(dag_bf16x8, X)
template <bool SPLIT>
__device__ __forceinline__ void dag_seg_sh(float* __restrict__ lds, const DagLane& L, const char* Ad, const char* Bd, int nkb, f32x16& acc00,
                                           f32x16& acc01, f32x16& acc10, f32x16& acc11) {
    constexpr int UPT = SPLIT ? 8 : 4;                          // units per tile
    constexpr int64_t USTEP = SPLIT ? kShGroup : 2 * kShGroup;  // bytes between a tile's units in the source
    constexpr int U = kShStageUnits, P = kShStagePieces;
    const int nst = __builtin_amdgcn_readfirstlane(nkb) * (UPT / U);    // stages; a multiple of kShRing (wave-uniform: the waits below are scalar branches)
    // fragment addresses: logical chunks fh and 2 + fh of the lane's row of each operand, in unit slot 0
    typedef __attribute__((address_space(3))) const void* lcptr_t;
    const unsigned sw = 16 * (L.fh ^ ((L.frow >> 2) & 3));
    const unsigned a_row = (unsigned)(uintptr_t)(lcptr_t)lds + (L.wr * 64 + L.frow) * 64;
    const unsigned b_row = (unsigned)(uintptr_t)(lcptr_t)lds + kShUnit / 2 + (L.wc * 64 + L.frow) * 64;
    const unsigned a_q0 = a_row + sw, a_q1 = a_row + (sw ^ 32u), b_q0 = b_row + sw, b_q1 = b_row + (sw ^ 32u);
    auto issue = [&](int s) {                                   // stage s into its ring slot
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int n = s * U + u;                            // unit n of the segment
            const int64_t off = (int64_t)(n / UPT) * kShTile + (n % UPT) * USTEP;
            dag_sh_dma(lds, (s % kShRing) * U + u, L, Ad + off, Bd + off);
        }
    };
    auto unit = [&](auto us, unsigned turn) {                   // the k-chunk(s) of the unit in unit slot `us` (+ turn bytes)
        constexpr int O = decltype(us)::value * kShUnit;
        const unsigned pa0 = a_q0 + turn, pa1 = a_q1 + turn, pb0 = b_q0 + turn, pb1 = b_q1 + turn;
        dag_u32x4 a0 = dag_lds_rd<O>(pa0), a1 = dag_lds_rd<O + 32 * 64>(pa0);
        dag_u32x4 b0 = dag_lds_rd<O>(pb0), b1 = dag_lds_rd<O + 32 * 64>(pb0);
        dag_u32x4 c0 = dag_lds_rd<O>(pa1), c1 = dag_lds_rd<O + 32 * 64>(pa1);
        dag_u32x4 d0 = dag_lds_rd<O>(pb1), d1 = dag_lds_rd<O + 32 * 64>(pb1);
        if (!SPLIT) {                                           // two k-chunks: (a, b), then (c, d)
            dag_lds_wait<4>(a0, a1, b0, b1);                    // (LDS reads return in order)
            DAG_MFMA4_BF16(a0, a1, b0, b1)
            dag_lds_wait<0>(c0, c1, d0, d1);
            DAG_MFMA4_BF16(c0, c1, d0, d1)
        } else {                                                // one k-chunk: a, b = hi, c, d = lo
            dag_lds_wait_all(a0, a1, b0, b1, c0, c1, d0, d1);
            DAG_MFMA4_BF16(c0, c1, b0, b1)
            DAG_MFMA4_BF16(a0, a1, d0, d1)
            DAG_MFMA4_BF16(a0, a1, b0, b1)
        }
    };
    auto phase = [&](auto r, int s, unsigned turn) {            // stage s, in ring slot r + (turn ? kShRing / 2 : 0)
        constexpr int R = decltype(r)::value;
        if (s + kShAhead < nst) issue(s + kShAhead);
        unit(DagInt<R * U>{}, turn);
        if constexpr (U == 2) unit(DagInt<R * U + U - 1>{}, turn);
        const int left = nst - 2 - s;                           // stages behind s + 1 that exist
        if (left >= kShAhead - 1) dag_vm_wait<P * (kShAhead - 1)>();
        else if (kShAhead >= 3 && left == 1) dag_vm_wait<P>();
        else dag_vm_wait<0>();
        dag_ring_barrier();
    };
#pragma unroll
    for (int s = 0; s < kShAhead; ++s) issue(s);
    dag_vm_wait<P * (kShAhead - 1)>();
    dag_ring_barrier();
    for (int s = 0; s < nst; s += kShRing / 2) {                // half a turn, 32 KiB of the image, per iteration
        const unsigned turn = ((s / (kShRing / 2)) & 1) * 2 * kShUnit;
        phase(DagInt<0>{}, s, turn);
        if constexpr (kShRing == 4) phase(DagInt<1>{}, s + 1, turn);
    }
}
#undef DAG_MFMA4_BF16
#undef DAG_BF
__device__ __forceinline__ void dag_seg_bf16(float* __restrict__ lds, const DagLane& L, const float* Ad, int64_t lda, const float* Bd, int64_t ldb,
                                             int nkt, f32x16& acc00, f32x16& acc01, f32x16& acc10, f32x16& acc11) {
    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    constexpr int IMG = NB * BK;
#define DAG_DMA(buf, k0)                                                                                           \
    do {                                                                                                           \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                            \
            __builtin_amdgcn_global_load_lds((gptr_t)(Ad + (int64_t)(8 * i) * lda + (k0)),                         \
                                             (lptr_t)(lds + ((buf) * 2 + 0) * IMG + (L.wid * 32 + 8 * i) * BK), 16, 0, 0); \
            __builtin_amdgcn_global_load_lds((gptr_t)(Bd + (int64_t)(8 * i) * ldb + (k0)),                         \
                                             (lptr_t)(lds + ((buf) * 2 + 1) * IMG + (L.wid * 32 + 8 * i) * BK), 16, 0, 0); \
        }                                                                                                          \
    } while (0)
    // the 8 floats of k-chunk c of row `row` (an offset into an operand image), as two 16-byte reads
#define DAG_RD8(lo, hi, buf, op, row, c)                                                                                              \
    do {                                                                                                                              \
        lo = *reinterpret_cast<const float4*>(lds + ((buf) * 2 + (op)) * IMG + (row) + 4 * ((4 * (c) + 2 * L.fh) ^ L.sw));            \
        hi = *reinterpret_cast<const float4*>(lds + ((buf) * 2 + (op)) * IMG + (row) + 4 * ((4 * (c) + 2 * L.fh + 1) ^ L.sw));        \
    } while (0)
#define DAG_CHUNK(buf, c)                                                                                          \
    do {                                                                                                           \
        float4 a0l, a0h, a1l, a1h, b0l, b0h, b1l, b1h;                                                             \
        DAG_RD8(a0l, a0h, buf, 0, L.arow, c);                                                                      \
        DAG_RD8(a1l, a1h, buf, 0, L.arow + 32 * BK, c);                                                            \
        DAG_RD8(b0l, b0h, buf, 1, L.brow, c);                                                                      \
        DAG_RD8(b1l, b1h, buf, 1, L.brow + 32 * BK, c);                                                            \
        const dag_bf16x8 a0 = dag_pack8(a0l, a0h), a1 = dag_pack8(a1l, a1h);                                       \
        const dag_bf16x8 b0 = dag_pack8(b0l, b0h), b1 = dag_pack8(b1l, b1h);                                       \
        acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc00, 0, 0, 0);                                   \
        acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc01, 0, 0, 0);                                   \
        acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc10, 0, 0, 0);                                   \
        acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc11, 0, 0, 0);                                   \
    } while (0)
    DAG_DMA(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nkt) DAG_DMA(cur ^ 1, (kt + 1) * BK);       // the other buffer is free since the last barrier
        DAG_CHUNK(cur, 0);
        DAG_CHUNK(cur, 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's DMA pieces of K-step kt+1 have landed ...
        __syncthreads();                                        // ... everyone else's too; every read of K-step kt is back
    }
#undef DAG_CHUNK
}
__device__ __forceinline__ void dag_seg_bf16x2(float* __restrict__ lds, const DagLane& L, const float* Ad, int64_t lda, const float* Bd, int64_t ldb,
                                               int nkt, f32x16& acc00, f32x16& acc01, f32x16& acc10, f32x16& acc11) {
    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    constexpr int IMG = NB * BK;
#define DAG_SPLIT(H, LO, buf, op, row, c)                                                                          \
    do {                                                                                                           \
        float4 rl, rh;                                                                                             \
        DAG_RD8(rl, rh, buf, op, row, c);                                                                          \
        dag_split8(rl, rh, H, LO);                                                                                 \
    } while (0)
#define DAG_CHUNK(buf, c)                                                                                          \
    do {                                                                                                           \
        dag_bf16x8 a0, a0l, a1, a1l, b0, b0l, b1, b1l;                                                             \
        DAG_SPLIT(a0, a0l, buf, 0, L.arow, c);                                                                     \
        DAG_SPLIT(a1, a1l, buf, 0, L.arow + 32 * BK, c);                                                           \
        DAG_SPLIT(b0, b0l, buf, 1, L.brow, c);                                                                     \
        DAG_SPLIT(b1, b1l, buf, 1, L.brow + 32 * BK, c);                                                           \
        acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0l, b0, acc00, 0, 0, 0);                                  \
        acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0l, b1, acc01, 0, 0, 0);                                  \
        acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1l, b0, acc10, 0, 0, 0);                                  \
        acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1l, b1, acc11, 0, 0, 0);                                  \
        acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0l, acc00, 0, 0, 0);                                  \
        acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1l, acc01, 0, 0, 0);                                  \
        acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0l, acc10, 0, 0, 0);                                  \
        acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1l, acc11, 0, 0, 0);                                  \
        acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc00, 0, 0, 0);                                   \
        acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc01, 0, 0, 0);                                   \
        acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc10, 0, 0, 0);                                   \
        acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc11, 0, 0, 0);                                   \
    } while (0)
    DAG_DMA(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nkt) DAG_DMA(cur ^ 1, (kt + 1) * BK);       // the other buffer is free since the last barrier
        DAG_CHUNK(cur, 0);
        DAG_CHUNK(cur, 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's DMA pieces of K-step kt+1 have landed ...
        __syncthreads();                                        // ... everyone else's too; every read of K-step kt is back
    }
#undef DAG_DMA
#undef DAG_RD8
#undef DAG_SPLIT
#undef DAG_CHUNK
}

// ... and as THREE-WAY split bf16 products -- the NEAR stretch of a bulk task's K-loop (knear, "Near stretch" at dag_task_order):
// fp32's 24 bits through the bf16 pipe.  Every operand fragment a becomes hi = bf16(a), mid = bf16(a - hi), lo = bf16(a - hi - mid)
// -- each rounded to nearest even by v_cvt_pk_bf16_f32, both differences exact in fp32; bf16 has fp32's exponent, so there is
// no range to mind and nothing is scaled; three parts of eight significant bits hold fp32's 24, so a = hi + mid + lo exactly
// (above bf16's denormal range) -- and a product a b^T becomes EIGHT, smallest terms first:  mid lo^T, lo mid^T, hi lo^T, lo hi^T,
// mid mid^T, hi mid^T, mid hi^T, hi hi^T.  Only lo lo^T is dropped, <= 2^-32 |a||b| per term.  (Six products, without the first
// two, were what the stretch was first written with: they lose up to 2^-23 of a term -- |mid| <= 2^-8 |a|, |lo| <= 2^-16 |a| at the
// bottom of a binade --, 2^-24.2 as measured, and miss the 2^-25 the stretch is specified with; they were 1.4 ms of the headline
// step faster.  The products are not what limits the stretch, though: with six OR eight the first residual of the headline's
// gain solve rises 10 - 13 % when every fp32 K-block takes it -- the bf16 pipe's accumulation of eight partial products per
// k-chunk is not the fp32 pipe's accumulation of exact products --, hence the cut-off kFactorNearBits, dense_tables.hip.)
// 32 MFMAs per k-chunk into the same four accumulators, term by term, the quadrants 00,
// 01, 10, 11 inside a term: no MFMA waits for the one in front of it.  1/2 of dag_seg's MFMA cycles per K-step (64 x 32
// against 64 x 64); the split is ~5.5 VALU instructions per operand element (11 per pair: three packs, four unpacks, four
// subtractions), operand by operand so that a raw fragment is dead before the next is split.
// The same fp32 LDS image, LDS-DMA fill and fragment addresses as dag_seg_bf16x2 -- nothing changes in memory -- but the
// fragment reads are written out (dag_lds_rd / dag_lds_wait, as in dag_seg_sh): left to the compiler the first ds_read of a
// K-step waits for vmcnt(0), i.e. for the DMA of the NEXT K-step issued just in front of it, which dag_seg hides behind 4 096
// MFMA cycles and this loop would not.  Here that DMA flies under the K-step's splits and MFMAs and is waited for once, in front
// of the barrier.  A k-chunk's B fragments are read first and split while its A fragments arrive; the next k-chunk's reads
// are issued before this one's MFMAs.  On entry no wave reads or fills the LDS image and this wave has no load in flight; on
// return everything has landed, every read is back and every wave is past a barrier, as after dag_seg.
__device__ __forceinline__ void dag_split2x3(unsigned x, unsigned y, unsigned& hi, unsigned& mid, unsigned& lo) {
    const float fx = __builtin_bit_cast(float, x), fy = __builtin_bit_cast(float, y);
    hi = dag_pk_bf16(fx, fy);
    const float rx = fx - __builtin_bit_cast(float, hi << 16), ry = fy - __builtin_bit_cast(float, hi & 0xffff0000u);
    mid = dag_pk_bf16(rx, ry);                                  // (= dag_pk_bf16_lo(fx, fy, hi): dag_split8's lo)
    lo = dag_pk_bf16_lo(rx, ry, mid);
}
__device__ __forceinline__ void dag_split8x3(const dag_u32x4& a, const dag_u32x4& b, dag_u32x4& hi, dag_u32x4& mid, dag_u32x4& lo) {
    unsigned h[4], m[4], l[4];
    dag_split2x3(a.x, a.y, h[0], m[0], l[0]);
    dag_split2x3(a.z, a.w, h[1], m[1], l[1]);
    dag_split2x3(b.x, b.y, h[2], m[2], l[2]);
    dag_split2x3(b.z, b.w, h[3], m[3], l[3]);
    hi = dag_u32x4{h[0], h[1], h[2], h[3]};
    mid = dag_u32x4{m[0], m[1], m[2], m[3]};
    lo = dag_u32x4{l[0], l[1], l[2], l[3]};
}
#define DAG_BF(X) __builtin_bit_cast(dag_bf16x8, X)
#define DAG_MFMA4_BF16(A0, A1, B0, B1)                                                          \
    acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(DAG_BF(A0), DAG_BF(B0), acc00, 0, 0, 0);    \
    acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(DAG_BF(A0), DAG_BF(B1), acc01, 0, 0, 0);    \
    acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(DAG_BF(A1), DAG_BF(B0), acc10, 0, 0, 0);    \
    acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(DAG_BF(A1), DAG_BF(B1), acc11, 0, 0, 0);
__device__ __forceinline__ void dag_seg_bf16x3(float* __restrict__ lds, const DagLane& L, const float* Ad, int64_t lda, const float* Bd, int64_t ldb,
                                               int nkt, f32x16& acc00, f32x16& acc01, f32x16& acc10, f32x16& acc11) {
    typedef __attribute__((address_space(3))) const void* lcptr_t;
    constexpr unsigned IMGB = NB * BK * 4;                      // bytes of one operand image; lds = [buf][A|B][image]
    // the lane's row of each operand in buffer 0, and the byte offsets of its four logical chunks 4 c + 2 fh + e inside the
    // 128-byte row: physical chunk = logical ^ sw, so they differ from the first by XORs of 16 (e) and 64 (c)
    const unsigned a_row = (unsigned)(uintptr_t)(lcptr_t)lds + 4u * (unsigned)L.arow;
    const unsigned b_row = (unsigned)(uintptr_t)(lcptr_t)lds + IMGB + 4u * (unsigned)L.brow;
    const unsigned q = 16u * (unsigned)((2 * L.fh) ^ L.sw);
    dag_u32x4 a0h, a0m, a0l, a1h, a1m, a1l, b0h, b0m, b0l, b1h, b1m, b1l;
    dag_u32x4 rb0, rb1, rb2, rb3, ra0, ra1, ra2, ra3;
    auto read = [&](unsigned turn, unsigned c64) {              // k-chunk c of the buffer at `turn` bytes: B's fragments, then A's
        const unsigned pb = b_row + turn, pa = a_row + turn, e0 = q ^ c64, e1 = e0 ^ 16u;
        rb0 = dag_lds_rd<0>(pb + e0); rb1 = dag_lds_rd<0>(pb + e1);
        rb2 = dag_lds_rd<32 * BK * 4>(pb + e0); rb3 = dag_lds_rd<32 * BK * 4>(pb + e1);
        ra0 = dag_lds_rd<0>(pa + e0); ra1 = dag_lds_rd<0>(pa + e1);
        ra2 = dag_lds_rd<32 * BK * 4>(pa + e0); ra3 = dag_lds_rd<32 * BK * 4>(pa + e1);
    };
    auto split = [&]() {
        dag_lds_wait<4>(rb0, rb1, rb2, rb3);                    // (LDS reads return in order)
        dag_split8x3(rb0, rb1, b0h, b0m, b0l);
        dag_split8x3(rb2, rb3, b1h, b1m, b1l);
        dag_lds_wait<0>(ra0, ra1, ra2, ra3);
        dag_split8x3(ra0, ra1, a0h, a0m, a0l);
        dag_split8x3(ra2, ra3, a1h, a1m, a1l);
    };
    auto products = [&]() {
        DAG_MFMA4_BF16(a0m, a1m, b0l, b1l)
        DAG_MFMA4_BF16(a0l, a1l, b0m, b1m)
        DAG_MFMA4_BF16(a0h, a1h, b0l, b1l)
        DAG_MFMA4_BF16(a0l, a1l, b0h, b1h)
        DAG_MFMA4_BF16(a0m, a1m, b0m, b1m)
        DAG_MFMA4_BF16(a0h, a1h, b0m, b1m)
        DAG_MFMA4_BF16(a0m, a1m, b0h, b1h)
        DAG_MFMA4_BF16(a0h, a1h, b0h, b1h)
    };
    const int n = __builtin_amdgcn_readfirstlane(nkt);
    dag_dma(lds, 0, L, (const char*)Ad, 4 * lda, (const char*)Bd, 4 * ldb);
    dag_vm_wait<0>();
    dag_ring_barrier();
    for (int kt = 0; kt < n; ++kt) {
        const int cur = kt & 1;
        const unsigned turn = (unsigned)cur * 2u * IMGB;
        if (kt + 1 < n)                                         // the other buffer is free since the last barrier
            dag_dma(lds, cur ^ 1, L, (const char*)(Ad + (kt + 1) * BK), 4 * lda, (const char*)(Bd + (kt + 1) * BK), 4 * ldb);
        read(turn, 0u);
        split();
        read(turn, 64u);                                        // (the raw fragments are dead: the second k-chunk's arrive under the first one's MFMAs)
        products();
        split();
        products();
        dag_vm_wait<0>();                                       // this wave's DMA pieces of K-step kt + 1 have landed ...
        dag_ring_barrier();                                     // ... everyone else's too; every read of K-step kt is back
    }
}
#undef DAG_MFMA4_BF16
#undef DAG_BF

// The writer: the final tile held in the accumulators -> its two planes at `tile` (a shadow tile).  Through LDS, so that the
// stores are coalesced 16-byte ones: a wave's 64 x 64 quadrant is rows 64 wr .. + 63 of the groups 4 wc .. + 3 of each plane,
// four runs of 2 KiB contiguous in memory, and it stages them -- [group][row][16 columns], the memory order -- in the two 8 KiB
// pieces of the image that dag_acc_to_image gives the same wave.  Banks of the 2-byte staging writes (32 banks of 4 bytes, by
// enumeration of a write's 64 lanes): 16 consecutive lanes share 8 banks pairwise in one dword; lanes frow and frow + 16 are
// 2 KiB apart and fh = 0, 1 are 128 bytes apart, both multiples of the 128-byte bank row -- 4 dwords per bank where the
// [row][64 columns] staging this replaced had 2.  Not swizzled away: the staging order is the memory order so that the
// reads below stay linear; the cost shows in the chain's panel phase and the tile tasks' tail, both reported with the ring
// (profiles/EXPERIMENTS.md, "A ring of four stages")
// (disjoint between waves: no barrier, the wave's own LDS accesses complete in order).  Every element is rounded as the
// in-loop variants round it: hi by v_cvt_pk_bf16_f32 (nearest even), lo = the same rounding of a - float(hi).  Stores are
// write-through (`sc1`) like the epilogue's and are drained by the vmcnt(0) of the caller's dag_publish.  On entry no wave
// reads or fills the LDS image; on return this wave's staging reads are complete.
__device__ __forceinline__ void dag_shadow_store(float* __restrict__ lds, const DagLane& L, char* tile, const f32x16& acc00, const f32x16& acc01,
                                                 const f32x16& acc10, const f32x16& acc11) {
    constexpr int IMG = NB * BK;
    unsigned short* hi = reinterpret_cast<unsigned short*>(lds + (L.wc * 2) * IMG + L.wr * (IMG / 2));
    unsigned short* lo = reinterpret_cast<unsigned short*>(lds + (L.wc * 2 + 1) * IMG + L.wr * (IMG / 2));
#define DAG_SH_PUT(ACC, i, j)                                                                           \
    _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                    \
        const int at = ((j) * 2 + (L.frow >> 4)) * 1024 + ((i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * L.fh) * 16 + (L.frow & 15); \
        const float a = ACC[e];                                                                         \
        const unsigned h = dag_pk_bf16(a, a);                                                           \
        const float rest = a - __builtin_bit_cast(float, h << 16);                                      \
        hi[at] = (unsigned short)h;                                                                     \
        lo[at] = (unsigned short)dag_pk_bf16(rest, rest);                                               \
    }
    DAG_SH_PUT(acc00, 0, 0)
    DAG_SH_PUT(acc01, 0, 1)
    DAG_SH_PUT(acc10, 1, 0)
    DAG_SH_PUT(acc11, 1, 1)
#undef DAG_SH_PUT
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // (also keeps the compiler from moving the reads below over the 2-byte writes)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)tile, (short)0, (int)kShTile, 0x00020000);
    const int voff = L.wc * 4 * kShGroup + L.wr * (kShGroup / 2) + L.lane * 16;
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        const dag_u32x4 vh = *reinterpret_cast<const dag_u32x4*>(reinterpret_cast<const char*>(hi) + n * 1024 + L.lane * 16);
        const dag_u32x4 vl = *reinterpret_cast<const dag_u32x4*>(reinterpret_cast<const char*>(lo) + n * 1024 + L.lane * 16);
        __builtin_amdgcn_raw_buffer_store_b128(vh, rs, voff, (n >> 1) * kShGroup + (n & 1) * 1024, 16);
        __builtin_amdgcn_raw_buffer_store_b128(vl, rs, voff, kShPlane + (n >> 1) * kShGroup + (n & 1) * 1024, 16);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the staging reads are back: the pieces may be rewritten
}

// The tile held in the accumulators becomes the operand image of a 128x128x128 product with ITSELF (the chain's rank-128
// update L(j+1,j) L(j+1,j)^T): element (row r, column c) goes to K-step image c / 32 at the swizzled position the fragment reads
// expect -- the four images fill the workgroup's LDS exactly -- and after a barrier every wave accumulates from LDS alone.
__device__ __forceinline__ void dag_acc_to_image(float* __restrict__ lds, const DagLane& L, const f32x16& acc00, const f32x16& acc01,
                                                 const f32x16& acc10, const f32x16& acc11) {
    constexpr int IMG = NB * BK;
    const int ch = L.frow >> 2, w = L.frow & 3;
#define DAG_PUT(ACC, i, j)                                                                              \
    _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                    \
        const int r = L.wr * 64 + (i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * L.fh;                         \
        lds[(L.wc * 2 + (j)) * IMG + r * BK + 4 * (ch ^ (r & 7)) + w] = ACC[e];                         \
    }
    DAG_PUT(acc00, 0, 0)
    DAG_PUT(acc01, 0, 1)
    DAG_PUT(acc10, 1, 0)
    DAG_PUT(acc11, 1, 1)
#undef DAG_PUT
}

__device__ __forceinline__ void dag_self_product(const float* __restrict__ lds, const DagLane& L, f32x16& acc00, f32x16& acc01, f32x16& acc10,
                                                 f32x16& acc11) {
    constexpr int IMG = NB * BK;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float* img = lds + s * IMG;
            const float4 a0 = *reinterpret_cast<const float4*>(img + L.arow + 4 * ((2 * g + L.fh) ^ L.sw));
            const float4 a1 = *reinterpret_cast<const float4*>(img + L.arow + 32 * BK + 4 * ((2 * g + L.fh) ^ L.sw));
            const float4 b0 = *reinterpret_cast<const float4*>(img + L.brow + 4 * ((2 * g + L.fh) ^ L.sw));
            const float4 b1 = *reinterpret_cast<const float4*>(img + L.brow + 32 * BK + 4 * ((2 * g + L.fh) ^ L.sw));
            DAG_MFMA16(a0, a1, b0, b1)
        }
    }
}

// epilogue of a tile held in the accumulators (C/D layout: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5) per
// 32x32 quadrant).  SUB: C <- C - acc, else C <- acc.  Loads of C and all stores are `sc1` (aux 16): see "L1 hygiene".
template <bool SUB>
__device__ __forceinline__ void dag_epilogue(float* Cg /* the wave's 64x64 quadrant */, int64_t ldc, const DagLane& L, const f32x16& acc00,
                                             const f32x16& acc01, const f32x16& acc10, const f32x16& acc11) {
    const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc((void*)Cg, (short)0, (int)(64 * ldc * 4), 0x00020000);
    const int cvoff = (int)(((4 * L.fh) * ldc + L.frow) * 4);
#define DAG_SOFF(i, j, e) (int)((((i) * 32 + ((e) & 3) + 8 * ((e) >> 2)) * ldc + (j) * 32) * 4)
#define DAG_EPI(ACC, i, j)                                                                                              \
    do {                                                                                                                \
        float pre[16];                                                                                                  \
        if (SUB) {                                                                                                      \
            _Pragma("unroll") for (int e = 0; e < 16; ++e)                                                              \
                pre[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(crs, cvoff, DAG_SOFF(i, j, e), 16)); \
        }                                                                                                               \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                                \
            const float o = SUB ? pre[e] - ACC[e] : ACC[e];                                                             \
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o), crs, cvoff, DAG_SOFF(i, j, e), 16);  \
        }                                                                                                               \
    } while (0)
    DAG_EPI(acc00, 0, 0);
    DAG_EPI(acc01, 0, 1);
    DAG_EPI(acc10, 1, 0);
    DAG_EPI(acc11, 1, 1);
#undef DAG_EPI
#undef DAG_SOFF
}

// bulk task on tile (i, j) of system sy: kind DAG_TILE (i >= j + 2: k < j, then the panel product, publishes rowfin[i] = j + 1),
// DAG_SUB (i = j + 1: k < j, leaves the updated tile, publishes sub[j]), DAG_PRE (i = j: k < j - 1, publishes pre[j]).
// k0 (wave-uniform, from the ticket): the K-loop's first block column -- 0, or first[i] of an ENVELOPED system ("Envelope" at
// dag_task_order): the blocks left of it are exact zeros that nobody wrote or reads, final by definition.
// kfar (wave-uniform, from the ticket, k0 <= kfar <= kend): the block columns k0 .. kfar - 1 are the row's FAR stretch -- every
// correlation between an observation of block row i and one of those block columns is below the far cut-off -- and their
// K-blocks run on the bf16 pipe (dag_seg_bf16); FAR = false (the launch that also solves): the ticket's kfar is ignored.
// kmid (wave-uniform, one scalar load from sy.mid per task, kfar <= kmid <= kend; no table: kfar): the block columns
// kfar .. kmid - 1 are the row's MIDDLE stretch, split bf16 products (dag_seg_bf16x2); kmid .. kend - 1 run in fp32.
// FAR = false ignores it too.
// knear (wave-uniform, one scalar load from sy.near per task, kmid <= knear <= kend; no table: kmid): the block columns
// kmid .. knear - 1 are the row's NEAR stretch, three-way split bf16 products from the fp32 tiles (dag_seg_bf16x3); only
// knear .. kend - 1 run on the fp32 pipe.  FAR = false ignores it as well.
// With a shadow (sy.shadow, "Shadow" above; FAR only) the far and / or middle segments (sy.shuse) read the operands' bf16
// images instead, and a DAG_TILE task stores its tile's images in front of its publish.
template <bool FAR>
__device__ __forceinline__ bool dag_tile_task(const DagSys& sy, int kind, int k0, int kfar, int i, int j, DagCtl* ctl, float* lds, const DagLane& L,
                                              int* s_flag, int* s_kav, long long* tr /* thread 0, tracing: [2] += time spent polling */) {
    const int t = threadIdx.x;
    const int kend = kind == DAG_PRE ? j - 1 : j;
    int* const st = sy.state;
    const int* rowfin_i = st + DAG_STATE_HDR + i;
    const int* rowfin_j = st + DAG_STATE_HDR + j;
    const float* Arow = sy.S + (int64_t)i * NB * sy.ld;
    const float* Brow = sy.S + (int64_t)j * NB * sy.ld;
    f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
    // the operand rows' tiles in the shadow (tile k of row r: + k * kShTile), wave-uniform; null: the in-loop conversions
    const char* shA = nullptr;
    const char* shB = nullptr;
    if (FAR && sy.shadow) {
        shA = sy.shadow + sy.shrow[i] * kShTile;
        shB = sy.shadow + sy.shrow[j] * kShTile;
    }
    int kmid = kfar;
    if (FAR && sy.mid) {
        kmid = sy.mid[i];
        kmid = kmid < kfar ? kfar : kmid;
        kmid = kmid > kend ? (kend > kfar ? kend : kfar) : kmid;
    }
    int knear = kmid;
    if (FAR && sy.near) {
        knear = sy.near[i];
        knear = knear < kmid ? kmid : knear;
        knear = knear > kend ? (kend > kmid ? kend : kmid) : knear;
    }
    int k = k0;
    while (k < kend) {
        bool ok = true;
        if (t == 0) {                                           // how far are the two row panels final?
            const long long w0 = tr ? wall_clock64() : 0;
            ok = dag_wait_ge(rowfin_i, k + 1, ctl, L.spin) && (i == j || dag_wait_ge(rowfin_j, k + 1, ctl, L.spin));
            if (tr) tr[2] += wall_clock64() - w0;
            int a = __hip_atomic_load(rowfin_i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int b = i == j ? a : __hip_atomic_load(rowfin_j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a = a < b ? a : b;
            *s_kav = a < kend ? a : kend;
        }
        if (!dag_join(ok, s_flag)) return false;
        int kav = *s_kav;
        if (FAR && k < kfar) {                                  // a segment ends where the far stretch does
            kav = kav < kfar ? kav : kfar;
            if (shA && (sy.shuse & 1))
                dag_seg_sh<false>(lds, L, dag_sh_src<false>(shA + k * kShTile, L), dag_sh_src<false>(shB + k * kShTile, L), kav - k,
                                        acc00, acc01, acc10, acc11);
            else
                dag_seg_bf16(lds, L, dag_src(Arow + (int64_t)k * NB, sy.ld, L), sy.ld, dag_src(Brow + (int64_t)k * NB, sy.ld, L), sy.ld,
                             (kav - k) * (NB / BK), acc00, acc01, acc10, acc11);
        } else if (FAR && k < kmid) {                           // ... and where the middle stretch does
            kav = kav < kmid ? kav : kmid;
            if (shA && (sy.shuse & 2))
                dag_seg_sh<true>(lds, L, dag_sh_src<true>(shA + k * kShTile, L), dag_sh_src<true>(shB + k * kShTile, L), kav - k,
                                       acc00, acc01, acc10, acc11);
            else
                dag_seg_bf16x2(lds, L, dag_src(Arow + (int64_t)k * NB, sy.ld, L), sy.ld, dag_src(Brow + (int64_t)k * NB, sy.ld, L), sy.ld,
                               (kav - k) * (NB / BK), acc00, acc01, acc10, acc11);
        } else if (FAR && k < knear) {                          // ... and the near one
            kav = kav < knear ? kav : knear;
            dag_seg_bf16x3(lds, L, dag_src(Arow + (int64_t)k * NB, sy.ld, L), sy.ld, dag_src(Brow + (int64_t)k * NB, sy.ld, L), sy.ld,
                           (kav - k) * (NB / BK), acc00, acc01, acc10, acc11);
        } else {
            dag_seg(lds, L, dag_src(Arow + (int64_t)k * NB, sy.ld, L), sy.ld, dag_src(Brow + (int64_t)k * NB, sy.ld, L), sy.ld, (kav - k) * (NB / BK),
                    acc00, acc01, acc10, acc11);
        }
        k = kav;
        __syncthreads();                                        // s_kav / s_flag may be rewritten
    }
    float* Ct = sy.S + (int64_t)i * NB * sy.ld + (int64_t)j * NB;
    float* Cq = Ct + (int64_t)(L.wr * 64) * sy.ld + L.wc * 64;
    if (kind != DAG_TILE) {
        dag_epilogue<true>(Cq, sy.ld, L, acc00, acc01, acc10, acc11);
        // the tile's lines in this CU's L1 hold what the `sc1` loads fetched or what these stores wrote -- not what the chain
        // will make of the tile: drop them, AFTER the last wave's last access (the barrier), before anybody is told
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) {
            asm volatile("buffer_inv sc1\n\ts_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(st + DAG_STATE_HDR + (kind == DAG_PRE ? sy.nb : 2 * sy.nb) + j, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return true;
    }
    if (kend > k0) {                                            // X = S(i,j) - acc back to the tile: the panel product reads it as an operand
        dag_epilogue<true>(Cq, sy.ld, L, acc00, acc01, acc10, acc11);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    bool ok = true;
    if (t == 0) {                                               // diagonal block j: T_j is published
        const long long w0 = tr ? wall_clock64() : 0;
        ok = dag_wait_ge(st, j + 1, ctl, L.spin);
        if (tr) { tr[2] += wall_clock64() - w0; tr[3] = wall_clock64(); }
    }
    if (!dag_join(ok, s_flag)) return false;                    // (its barrier: every wave's X is out)
    acc00 = f32x16{0}; acc01 = f32x16{0}; acc10 = f32x16{0}; acc11 = f32x16{0};
    dag_seg(lds, L, dag_src(Ct, sy.ld, L), sy.ld, dag_src(sy.tinv + (int64_t)j * NB * NB, NB, L), NB, NB / BK, acc00, acc01, acc10, acc11);
    if (t == 0) dag_drop_l1();                                  // this CU's L1 holds lines of X where L(i,j) is about to be
    dag_epilogue<false>(Cq, sy.ld, L, acc00, acc01, acc10, acc11);
    if (FAR && sy.shadow) dag_shadow_store(lds, L, sy.shadow + (sy.shrow[i] + j) * kShTile, acc00, acc01, acc10, acc11);     // (the K-segment's last barrier is behind every wave)
    dag_publish(st + DAG_STATE_HDR + i, j + 1);
    return true;
}

// A chain step, first half: the diagonal-block waves on tile (j,j) (complete in S), publish diagdone
__device__ __forceinline__ void dag_chain_diag(const DagSys& sy, int j, int* info, float* lds, const DagLane& L, const struct DagSolve* sv,
                                               struct DagCtl* ctl);
__device__ __forceinline__ void dag_chain_diag_body(const DagSys& sy, int j, int* info, float* lds, const DagLane& L, bool* announced) {
    // LDS of the diagonal-block waves, inside the GEMM image (never live at the same time)
    float* Pp = lds;
    float* Xr = Pp + 2 * D3_PBUF;
    float* dinvb = Xr + 7 * D3_TILE;
    float* stage = dinvb + 2 * D3_TILE;
    // The waves' tile addresses are functions of (ld, lane) only: left to itself the compiler computes all of them in front of
    // the caller's j loop and keeps them live across it (256 VGPRs and 40 spilled, where the stand-alone kernel needs 95).
    // Passing the three inputs through an empty asm makes them this call's values.
    int64_t ldj = sy.ld;
    int lrj = L.lane & 15, lgj = L.lane >> 4;
    asm volatile("" : "+s"(ldj), "+v"(lrj), "+v"(lgj));
    gfloat* Sb = (gfloat*)(sy.S + (int64_t)j * NB * sy.ld + (int64_t)j * NB);
    gfloat* Tg = (gfloat*)(sy.tinv + (int64_t)j * NB * NB);
    if (L.wid == 0) d3_diagonal_wave<true>(Sb, ldj, Pp, dinvb, stage, info, j * NB, L.lane, lrj, lgj, sy.which);
    else if (L.wid == 1) d3_worker_wave<1, true>(Sb, ldj, Tg, Pp, Xr, dinvb, stage, lrj, lgj);
    else if (L.wid == 2) d3_worker_wave<2, true>(Sb, ldj, Tg, Pp, Xr, dinvb, stage, lrj, lgj);
    else d3_worker_wave<3, true>(Sb, ldj, Tg, Pp, Xr, dinvb, stage, lrj, lgj);
    *announced = true;
#ifdef OISAT_TEST_HOOKS
    if ((L.flags & 128) && j >= 3) {                            // (fault injection: from block 3 on the diagonal blocks are never announced)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        *announced = false;
        return;
    }
#endif
    dag_publish(sy.state, j + 1);                               // diagdone: L(j,j) and T_j are out
}

// A chain step, second half (sub(j) is set; the barrier of the caller's join is behind us): panel tile L(j+1,j) = S(j+1,j) T_j^T,
// stored and handed to LDS as an operand image, publish rowfin[j+1]; rank-128 update of (j+1,j+1) from LDS; poll
// pre(j+1) only now (a dedicated chain: the flag has had the whole panel product to arrive); write the tile back for the
// next block's waves.
template <bool SH /* the launch may carry a shadow (every instantiation but the one that also solves) */>
__device__ __forceinline__ bool dag_chain_panel(const DagSys& sy, int j, DagCtl* ctl, float* lds, const DagLane& L, int* s_flag, long long* ctr) {
    const int t = threadIdx.x;
    int* const st = sy.state;
    float* Sjj = sy.S + (int64_t)j * NB * sy.ld + (int64_t)j * NB;
    f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
    float* Pt = Sjj + (int64_t)NB * sy.ld;                      // tile (j+1, j)
    dag_seg(lds, L, dag_src(Pt, sy.ld, L), sy.ld, dag_src(sy.tinv + (int64_t)j * NB * NB, NB, L), NB, NB / BK, acc00, acc01, acc10, acc11);
    if (t == 0) dag_drop_l1();                                  // L1 holds the tile as SUB(j) left it
    dag_epilogue<false>(Pt + (int64_t)(L.wr * 64) * sy.ld + L.wc * 64, sy.ld, L, acc00, acc01, acc10, acc11);
    // the tile's shadow first: it stages in the very pieces of the image this wave fills next
    if (SH && sy.shadow) dag_shadow_store(lds, L, sy.shadow + (sy.shrow[j + 1] + j) * kShTile, acc00, acc01, acc10, acc11);
    dag_acc_to_image(lds, L, acc00, acc01, acc10, acc11);
    dag_publish(st + DAG_STATE_HDR + j + 1, j + 1);             // rowfin[j+1] (its barrier: the image is complete)
    if (ctr && t == 0) ctr[8 * j + 3] = wall_clock64();
    acc00 = f32x16{0}; acc01 = f32x16{0}; acc10 = f32x16{0}; acc11 = f32x16{0};
    dag_self_product(lds, L, acc00, acc01, acc10, acc11);
    if (ctr && t == 0) ctr[8 * j + 4] = wall_clock64();
    {
        bool ok = true;
        if (t == 0 && j >= 1) ok = dag_wait_ge(st + DAG_STATE_HDR + sy.nb + j + 1, 1, ctl, L.spin);       // pre(j+1)
        if (ctr && t == 0) ctr[8 * j + 5] = wall_clock64();
        if (!dag_join(ok, s_flag)) return false;
    }
    dag_epilogue<true>(Sjj + (int64_t)NB * sy.ld + NB + (int64_t)(L.wr * 64) * sy.ld + L.wc * 64, sy.ld, L, acc00, acc01, acc10, acc11);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                            // tile (j+1,j+1) is complete in memory; nobody reads the image any more
    return true;
}

// the chain of ONE system on a workgroup of its own (the systems with the most block rows: the launch ends with them)
template <bool SH>
__device__ __forceinline__ bool dag_chain_task(const DagSys& sy, DagCtl* ctl, int* info, float* lds, const DagLane& L, int* s_flag,
                                               long long* ctr /* tracing: [nb][8] stamps of this chain */, const struct DagSolve* sv) {
    const int t = threadIdx.x;
    __builtin_amdgcn_s_setprio(3);                              // where this workgroup shares its CU: the arbiter serves the chain first
    for (int j = 0; j < sy.nb; ++j) {
        if (ctr && t == 0) ctr[8 * j + 0] = wall_clock64();
#ifdef OISAT_TEST_HOOKS
        if (L.flags & 512)                                      // (profiling aid: every chain step ~5 us longer -- 4 x 47 x 64 clocks at 2.4 GHz)
            for (int n = 0; n < 4; ++n) __builtin_amdgcn_s_sleep(47);
#endif
        dag_chain_diag(sy, j, info, lds, L, sv, ctl);
        if (ctr && t == 0) ctr[8 * j + 1] = wall_clock64();
        if (j + 1 == sy.nb) break;
        bool ok = true;
        if (t == 0 && j >= 1) ok = dag_wait_ge(sy.state + DAG_STATE_HDR + 2 * sy.nb + j, 1, ctl, L.spin);   // sub(j)
        if (ctr && t == 0) ctr[8 * j + 2] = wall_clock64();
        if (!dag_join(ok, s_flag)) return false;       // (its barrier: the diagonal-block waves' LDS reads are over)
        if (!dag_chain_panel<SH>(sy, j, ctl, lds, L, s_flag, ctr)) return false;
    }
    __builtin_amdgcn_s_setprio(0);
    return true;
}

// ---- The solve phase as tasks ---------------------------------------------------------------------------------------------
// Why: behind a month's factorization launch sat a fully exposed solve phase -- four triangular sweeps at the HBM rate, two
// float64 residuals and the increment on the VALU, 12 of 62 ms with the MFMA pipes idle -- and a persistent launch that holds
// every workgroup slot cannot share the chip with other kernels (their LDS does not fit beside two 65 KB workgroups).  So
// the solve of a system becomes tasks of the SAME launch: drawn by the same workgroups between tile tasks, beside a tile task
// on the other slot of their CU (MFMA next to HBM streaming / VALU work); the solves of the systems that are factored first
// run under the factorization of the others, only the last ones' are exposed.
//   per system, per round r = 0 .. refine:   FWD(b, r) b = 0 .. nb-1  ->  BWD(b, r)  ->  RES(c, r) c = 0 .. m/64   [check]
//   then INC(patch).  The arithmetic of a task is the device function the stand-alone kernels call (trsv_row,
//   resid_*_block, increment_patch): per system the same numbers, bit for bit, as oisat_batch_potrf + oisat_batch_solve.
// READY QUEUE, not tickets.  A first version put the solve tasks into the ticket list (a wave's solve spread over the next
// wave's tickets) and let each wait for its input: 75 ms instead of 62 -- a workgroup that draws a task whose input is not
// there holds one of the 512 slots spinning (traced: 5.7 of the solve's 13.3 slot-seconds were polling).  Now a task enters a
// queue of the launch only when what it waits for is complete, pushed by the task that completes it: the chain pushes
// FWD(j, 0) when diagonal block j is out (the first forward sweep rides behind the factorization); the last row of a sweep to
// finish pushes all rows of the next sweep (a window of rows was tried: the sweep of a 137-block polar cap then runs at
// window x 32 GB/s instead of the HBM rate and takes 3 ms instead of 1); the last BWD row pushes the residual blocks -- and,
// behind a correction, the increment's patches (dag_push_increment) --, the last residual block forms the norm, decides and
// pushes the next round; the last patch of the final increment counts the system as done.  A workgroup looks into the
// queues before it draws a ticket; the launch ends when the tickets are gone and every system is done.  Inside a sweep rows
// still wait for their predecessors' payload (trsv_row) -- all of them pushed, and therefore claimed, earlier.
// WHAT IT BOUGHT (tools/dag_solve_trace.py, profiles/r04_*): a localised 720x1440 month 61.5-63 ms in one launch against
// 62.6 ms as factorization launch + lock-step solve launches; twelve months 0.73 against 0.71 s.  The launch is bound by
// workgroup-slot time: 22.9 slot-seconds of factorization tasks + 7.3 of solve tasks over 512 slots.  A tile task beside a
// solve task runs 1.5 x faster than beside another tile task (10.6 vs 16.2 us per 128-deep K-block) -- but the solve task
// beside it runs 1.4 x slower (a residual block 300 vs 221 us), and tools/corun3_probe.py shows the same from outside: a
// month's increments as a THIRD workgroup per CU beside the factorization-only launch (96 VGPRs / 27 KB: they fit) take
// exactly as long as the two one after the other (50.2 + 3 x 6.9 ms alone, 70.8 ms together).  fp64 VALU work and the fp32
// MFMA K-loop do not overlap on this chip to any useful degree; what is left of the solve phase has to be made SMALLER, not
// hidden.  The path stays (same bits as the lock-step solve, one launch instead of ~15) and is the caller's choice
// (oisat_batch_analyse); the Python package keeps the lock-step solve by default.
// Hand-overs (cdna_hip_programming.md Guideline 16): everything a task stores for another task is stored write-through at
// agent scope and drained before the counter add / queue push that announces it; a task starts with one agent acquire.
__device__ __forceinline__ int dag_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void dag_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Two queues: 0 holds the rows of the triangular sweeps -- short, latency-bound links of a dependent chain: every workgroup
// looks there first --, 1 the residual blocks and increment patches -- long VALU-bound tasks: only the SECOND workgroup of a
// CU takes them while tickets are left, so that a CU runs one of them beside a tile task (VALU next to MFMA: both at full
// speed) and not two of them beside each other with its MFMA pipe idle (traced: a polar cap's 720 patches, pushed at once,
// took 380 of the 512 slots and the tile tasks 50).
__device__ __forceinline__ int dag_queue_of(int kind) { return kind >= DAG_RES ? 1 : 0; }
// one thread: entry `slot` (of its queue) <- task.  The second word goes first and is acknowledged before the first, which is
// the one a consumer polls.
__device__ __forceinline__ void dag_queue_write(const DagSolve& sv, DagCtl* ctl, int qi, int slot, int kind, int sys, int a, int b) {
    if (slot >= (qi ? sv.qcap - sv.qcap0 : sv.qcap0)) {        // (the host sized the queues for every task of the launch)
        dag_st(&ctl->error, 1);
        return;
    }
    unsigned long long* e = sv.queue + 2 * (int64_t)((qi ? sv.qcap0 : 0) + slot);
    __hip_atomic_store(e + 1, (unsigned long long)(unsigned)a | ((unsigned long long)(unsigned)b << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(e, (unsigned long long)(unsigned)kind | ((unsigned long long)(unsigned)sys << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one thread pushes one task
__device__ __forceinline__ void dag_push_one(const DagSolve& sv, DagCtl* ctl, int kind, int sys, int a, int b) {
    const int qi = dag_queue_of(kind);
    const int slot = __hip_atomic_fetch_add(&ctl->q[qi].tail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    dag_queue_write(sv, ctl, qi, slot, kind, sys, a, b);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_fetch_add(&ctl->q[qi].avail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the whole workgroup pushes tasks (kind, sys, a0 .. a0 + n - 1, b); n is block-uniform
__device__ __forceinline__ void dag_push_many(const DagSolve& sv, DagCtl* ctl, int kind, int sys, int a0, int n, int b, int* s_base) {
    const int qi = dag_queue_of(kind);
    __syncthreads();
    if (threadIdx.x == 0) *s_base = __hip_atomic_fetch_add(&ctl->q[qi].tail, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int base = *s_base;
    for (int i = threadIdx.x; i < n; i += 256) dag_queue_write(sv, ctl, qi, base + i, kind, sys, a0 + i, b);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(&ctl->q[qi].avail, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// thread 0: claim the oldest ready task of queue qi; false = none there.  Every access of the claim is a read-modify-write:
// under a month's load an agent-scope LOAD of the queue's counters took ~100 us (it queues behind the sweeps' polling loads
// at the memory side -- traced: a third of every workgroup's life went into looking at an empty queue), an RMW 3 us.
// avail = entries written and not yet claimed (a semaphore); head = the next entry to hand out.
__device__ __forceinline__ bool dag_queue_pop(const DagSolve& sv, DagCtl* ctl, int qi, int4* task_out, int* slot_out, long long* tm /* tracing: [look, claim, entry] */) {
    const long long c0 = tm ? wall_clock64() : 0;
    bool some = __hip_atomic_fetch_add(&ctl->q[qi].avail, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0;
    if (some && __hip_atomic_fetch_add(&ctl->q[qi].avail, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= 0) {
        __hip_atomic_fetch_add(&ctl->q[qi].avail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // lost a race for the last entries: give it back
        some = false;
    }
    if (!some) {
        if (tm) tm[0] += wall_clock64() - c0;
        return false;
    }
    int h = __hip_atomic_fetch_add(&ctl->q[qi].head, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long c1 = tm ? wall_clock64() : 0;
    if (tm) tm[1] += c1 - c0;
    if (h >= (qi ? sv.qcap - sv.qcap0 : sv.qcap0)) return false;
    h += qi ? sv.qcap0 : 0;
    unsigned long long w0;
    unsigned spins = 0;
    while (((w0 = __hip_atomic_load(&sv.queue[2 * (int64_t)h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & 0xffffffffull) == 0ull) {
        __builtin_amdgcn_s_sleep(1);                            // (its writer is between the reservation and the store)
        if (++spins > (1u << 22)) {
            dag_st(&ctl->error, 1);
            return false;
        }
    }
    const unsigned long long w1 = __hip_atomic_load(&sv.queue[2 * (int64_t)h + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *task_out = int4{(int)(w0 & 0xffffffffull), (int)(w0 >> 32), (int)(w1 & 0xffffffffull), (int)(w1 >> 32)};
    *slot_out = h;
    if (tm) tm[2] += wall_clock64() - c1;
    return true;
}

__device__ __forceinline__ int dag_inc_patches(const SolveMember& mb, int cells) {
    if (mb.nx > 0) return (int)(((mb.nx + 31) / 32) * (((mb.n / mb.nx) + 8 * cells - 1) / (8 * cells)));
    return (int)((mb.n + 256 * cells - 1) / (256 * cells));
}

// a chain step, first half, in a launch that also solves: diagonal block j is out -> row j of the first forward sweep is ready
__device__ __forceinline__ void dag_chain_diag(const DagSys& sy, int j, int* info, float* lds, const DagLane& L, const DagSolve* sv, DagCtl* ctl) {
    bool announced = false;
    dag_chain_diag_body(sy, j, info, lds, L, &announced);
    if (sv != nullptr && announced && threadIdx.x == 0) dag_push_one(*sv, ctl, DAG_FWD, sy.which, j, 0);
}

// whole workgroup, start of a solve task: one agent acquire (what the pusher announced is stored write-through)
__device__ __forceinline__ void dag_task_acquire() {
    if (threadIdx.x == 0) asm volatile("buffer_inv sc1\n\ts_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// The increment is pushed as soon as z is PROBABLY final -- behind the first correction, next to the residual evaluation that
// will say so -- instead of behind that evaluation's verdict: on every BASELINE workload one correction converges, and the
// evaluation + check would otherwise sit on every system's critical path (and all increments at the end of the launch).
// "Generation" g = the round whose z the patches use.  If the verdict is "not converged", round g + 1 follows and its
// increment -- pushed once generation g's patches are all through -- overwrites the fields.  A system counts as done when
// the patches of its FINAL generation are through: the patches add 1 to the generation's word, whoever learns that the
// generation is final adds DAG_INC_DECIDED, and the add that completes the sum reports the system.
__device__ __forceinline__ void dag_inc_account(int* word, int add, int npatch, DagCtl* ctl) {     // one thread
    const int v = __hip_atomic_fetch_add(word, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + add;
    if (v == DAG_INC_DECIDED + npatch) __hip_atomic_fetch_add(&ctl->sys_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// whole workgroup: push generation g of the system's increment (final: it is known to be the last one)
__device__ __forceinline__ bool dag_push_increment(const DagSys& sy, const SolveMember& mb, int sys, int g, bool final, const DagSolve& sv, DagCtl* ctl,
                                                   int* s_base, unsigned spin_max) {
    const int npatch = dag_inc_patches(mb, sv.cells);
    if (g >= 2) {                                               // (only behind a verdict "not converged": rare)  the previous generation's
        __syncthreads();                                        // patches must be through before these overwrite their fields
        if (threadIdx.x == 0) {
            unsigned spins = 0;
            int ok = 1;
            while ((__hip_atomic_fetch_add(sy.state + DAG_ST_INC + g - 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & (DAG_INC_DECIDED - 1)) < npatch) {
                __builtin_amdgcn_s_sleep(8);
                if (++spins > spin_max || dag_ld(&ctl->error) != 0) {
                    dag_st(&ctl->error, 1);
                    ok = 0;
                    break;
                }
            }
            *s_base = ok;
        }
        __syncthreads();
        const bool ok = *s_base != 0;
        __syncthreads();
        if (!ok) return false;
    }
    dag_push_many(sv, ctl, DAG_INC, sys, 0, npatch, g, s_base);
    if (final && threadIdx.x == 0) dag_inc_account(sy.state + DAG_ST_INC + g, DAG_INC_DECIDED, npatch, ctl);
    return true;
}

// z of `round` is complete (the last BWD row of the round, or the plain solve): what follows
__device__ __forceinline__ bool dag_after_sweeps(const DagSys& sy, const SolveMember& mb, int sys, int round, const DagSolve& sv, DagCtl* ctl, int* s_base,
                                                 unsigned spin_max) {
    const bool final = sv.refine == 0 || round == sv.refine;
    if (final || round >= 1)                                    // (the plain solve alone rarely meets the tolerance: no increment from it yet)
        if (!dag_push_increment(sy, mb, sys, round, final, sv, ctl, s_base, spin_max)) return false;
    if (sv.refine > 0) dag_push_many(sv, ctl, DAG_RES, sys, 0, (int)((mb.m + 63) / 64), round, s_base);      // (round = refine: the check behind the last correction)
    return true;
}

// The sweep tasks hand trsv_row this launch's control block as a TrsvCtl: it reads and raises `error`, nothing else
// (dense_trsv.inc: TrsvCtl), and that word is the same one in both blocks.
static_assert(offsetof(DagCtl, error) == offsetof(TrsvCtl, error) && sizeof(DagCtl::error) == sizeof(TrsvCtl::error),
              "trsv_row's error word is the launch's");

// one block row of a triangular sweep of round r; tk = its claim order (fwd: block row tk, bwd: block row nb - 1 - tk)
template <int TRANSPOSE>
__device__ __forceinline__ bool dag_sweep_task(const DagSys& sy, const SolveMember& mb, int sys, int tk, int round, const DagSolve& sv, DagCtl* ctl,
                                               float* lds, int* s_kav, unsigned spin_max) {
    const int t = threadIdx.x;
    int* const st = sy.state;
    const int nb = sy.nb;
    dag_task_acquire();
    __builtin_amdgcn_s_setprio(2);                              // a hop of a sweep is latency: first in line at the SIMD it shares with a tile task
    float* tile = lds;
    double* vec = reinterpret_cast<double*>(lds + NB * TLD);
    double* part = vec + NB;
    unsigned* s_ok = reinterpret_cast<unsigned*>(part + NB);
    if (t == 0) *s_ok = 1u;
    __syncthreads();
    double* in = TRANSPOSE ? mb.fwd : mb.rhs;
    double* out = TRANSPOSE ? mb.rhs : mb.fwd;
    if (!trsv_row<TRANSPOSE, true>(mb.S, mb.ld, mb.tinv, nb, tk, 0, in, out, reinterpret_cast<TrsvCtl*>(ctl), sv.trsv_timeouts, 0,
                                   TRANSPOSE ? mb.z : (double*)nullptr, mb.m, round > 0 ? 1 : 0, tile, vec, part, s_ok)) {
        __builtin_amdgcn_s_setprio(0);
        return false;
    }
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this row's stores (solution, re-armed input, z) are out ...
    __syncthreads();
    if (t == 0) {                                               // ... before it counts as through
        const int done = __hip_atomic_fetch_add(st + (TRANSPOSE ? DAG_ST_BWD : DAG_ST_FWD) + round, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *s_kav = done == nb - 1 ? 1 : 0;
    }
    __syncthreads();
    const bool last = *s_kav != 0;
    __syncthreads();
    if (last) {
        if (!TRANSPOSE) dag_push_many(sv, ctl, DAG_BWD, sys, 0, nb, round, s_kav);
        else if (!dag_after_sweeps(sy, mb, sys, round, sv, ctl, s_kav, spin_max)) return false;
    }
    return true;
}

// Row `row` of the FIRST forward sweep in the launch that factors one system and does nothing else of its solve
// (DAG_SOLVE_FWD).  Why this one sweep and nothing more: it needs only d, known before the launch, and row `row` of L, final
// when diagonal block `row` is out -- the chain pushes it then -- and it is HBM streaming, not VALU work: a row costs ~0.1 ms of
// one workgroup slot where the sweep as a launch of its own is a fully exposed chain of nb hand-overs (4 ms of the headline step).
// The float64 residual and the increment stay outside (they do not overlap with the K-loop: "WHAT IT BOUGHT" above), and the
// other sweeps wait for them.  An enveloped row starts at first[row] like trsv_pipe_kernel's (clamped the same way): the
// blocks left of it are the build's zeros.  The arithmetic is trsv_row's: the bits of the stand-alone sweep.  The last row to
// finish counts the system as done; nothing is pushed behind it.
__device__ __forceinline__ bool dag_fwd_row_task(const DagSys& sy, int row, const DagSolve& sv, DagCtl* ctl, float* lds) {
    dag_task_acquire();
    __builtin_amdgcn_s_setprio(2);
    float* tile = lds;
    double* vec = reinterpret_cast<double*>(lds + NB * TLD);
    double* part = vec + NB;
    unsigned* s_ok = reinterpret_cast<unsigned*>(part + NB);
    if (threadIdx.x == 0) *s_ok = 1u;
    __syncthreads();
    int step0 = 0;
    if (sv.env != nullptr) {
        step0 = sv.env[row];
        step0 = step0 < 0 ? 0 : (step0 > row ? row : step0);
    }
    const bool ok = trsv_row<0, true>(sy.S, sy.ld, sy.tinv, sy.nb, row, step0, sv.fwd_rhs, sv.fwd_sol, reinterpret_cast<TrsvCtl*>(ctl),
                                      sv.trsv_timeouts, 0, (double*)nullptr, (int64_t)0, 0, tile, vec, part, s_ok);
    __builtin_amdgcn_s_setprio(0);
    if (!ok) return false;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this row's stores (solution, re-armed right-hand side) are out ...
    __syncthreads();
    if (threadIdx.x == 0 &&                                     // ... before it counts as through
        __hip_atomic_fetch_add(sy.state + DAG_ST_FWD, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == sy.nb - 1)
        __hip_atomic_fetch_add(&ctl->sys_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// block c (64 rows) of residual evaluation e: r = d - S z into the padded right-hand side; the LAST block of an evaluation
// to finish forms |r|^2 (and |d|^2) in the order of resid_check_batched_kernel, publishes the verdict and pushes what follows
__device__ __forceinline__ bool dag_res_task(const DagSys& sy, const SolveMember& mb, int sys, int c, int e, const DagSolve& sv, DagCtl* ctl, int* info,
                                             float* lds, int* s_kav, unsigned spin_max) {
    const int t = threadIdx.x;
    int* const st = sy.state;
    dag_task_acquire();
    __builtin_amdgcn_s_setprio(1);                              // VALU work beside a tile task's MFMA wave: first at the issue port (the MFMA wave
    const SolveLds W = solve_lds_carve(lds);                    // issues one instruction per 64 cycles of its pipe and loses nothing)
    if (sv.blocks)
        resid_compact_block<OISAT_CORR_GAUSSIAN, true>(mb.oxyz, mb.osig, mb.ovar, mb.m, sv.g, mb.d, mb.z, mb.rhs, mb.olat, sv.win_deg, mb.perm, sv.cut_chord,
                                                       (sv.blocks & 2) ? (double)sv.far_chord : (double)INFINITY, (int64_t)c, W);
    else
        resid_rows_block<OISAT_CORR_GAUSSIAN, true>(mb.oxyz, mb.osig, mb.ovar, mb.m, sv.g, mb.d, mb.z, mb.rhs, sv.win_deg < 180.0 ? mb.olat : (const double*)nullptr,
                               sv.win_deg, (double*)nullptr, 1, 0, (int64_t)c, W);
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int nres = (int)((mb.m + 63) / 64);
    if (t == 0) *s_kav = __hip_atomic_fetch_add(st + DAG_ST_RES + e, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nres - 1 ? 1 : 0;
    __syncthreads();
    const bool last = *s_kav != 0;
    __syncthreads();
    if (!last) return true;
    // the check (resid_check_batched_kernel's arithmetic: 1024 strided partial sums, then a binary tree)
    dag_task_acquire();                                         // the other blocks' rows of r
    double* sr = reinterpret_cast<double*>(lds) + 4096;         // [1024] | [1024], behind the residual's carve-out (32 KB in)
    double* sd = sr + 1024;
    const double* r = mb.rhs;
    const double* d = mb.d;
    const int64_t m = mb.m;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double a = 0.0, b = 0.0;
        for (int64_t i = t + 256 * q; i < m; i += 1024) {
            a += r[i] * r[i];
            if (e == 0) b += d[i] * d[i];
        }
        sr[t + 256 * q] = a;
        sd[t + 256 * q] = b;
    }
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        for (int i = t; i < w; i += 256) {
            sr[i] += sr[i + w];
            sd[i] += sd[i + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        SolveState* ss = mb.st;
        double dd;
        if (e == 0) {
            dd = sd[0];
            __hip_atomic_store(&ss->dd, dd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            dd = __hip_atomic_load(&ss->dd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __hip_atomic_store(&ss->norm[e], sr[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        dag_st(&ss->computed, e + 1);
        const bool conv = sr[0] <= sv.tol2 * dd;
        if (conv) dag_st(&ss->conv, 1);
        else if (e == sv.refine && sv.tol2 > 0.0) {             // every allowed correction is in and the tolerance is not met
            atomicAdd(&info[kInfoUnconverged], 1);
            note_unconverged_member(&info[kInfoUnconvergedMember], mb.which);
        }
        *s_kav = conv ? 1 : 0;
    }
    __syncthreads();
    const bool conv = *s_kav != 0;
    __syncthreads();
    if (e < sv.refine) {                                        // (behind the last correction the increment is final anyway)
        if (conv && e == 0) {                                   // the plain solve met the tolerance: its increment, final
            if (!dag_push_increment(sy, mb, sys, 0, true, sv, ctl, s_kav, spin_max)) return false;
        } else if (conv) {                                      // generation e, on its way since round e's sweeps, is the final one
            if (t == 0) dag_inc_account(st + DAG_ST_INC + e, DAG_INC_DECIDED, dag_inc_patches(mb, sv.cells), ctl);
        } else {
            dag_push_many(sv, ctl, DAG_FWD, sys, 0, sy.nb, e + 1, s_kav);
        }
    }
    return true;
}

// patch `blk` of the system's increment (apply_increment_kernel's body); the last patch counts the system as done
template <typename T>
__device__ __forceinline__ bool dag_inc_task(const DagSys& sy, const SolveMember& mb, int blk, int gen, const DagSolve& sv, DagCtl* ctl, float* lds) {
    dag_task_acquire();
    __builtin_amdgcn_s_setprio(1);
    const SolveLds W = solve_lds_carve(lds);
    const bool windowed = sv.win_deg < 180.0;
    const double* glat = windowed ? mb.glat : (const double*)nullptr;
    const double* olat = windowed ? mb.olat : (const double*)nullptr;
    if (sv.cells == 1)
        increment_patch<OISAT_CORR_GAUSSIAN, T, 1>(mb.gxyz, mb.gsig, mb.n, mb.oxyz, mb.osig, mb.z, mb.m, sv.g2, (const T*)mb.xb, (T*)mb.xa, (T*)mb.inc, glat, olat,
                              sv.win_deg, mb.nx, sv.cut_chord, (double)sv.far_chord, (int64_t)blk, W);
    else
        increment_patch<OISAT_CORR_GAUSSIAN, T, 2>(mb.gxyz, mb.gsig, mb.n, mb.oxyz, mb.osig, mb.z, mb.m, sv.g2, (const T*)mb.xb, (T*)mb.xa, (T*)mb.inc, glat, olat,
                              sv.win_deg, mb.nx, sv.cut_chord, (double)sv.far_chord, (int64_t)blk, W);
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // (a later generation may overwrite these fields: this one's stores are out first)
    __syncthreads();
    if (threadIdx.x == 0) dag_inc_account(sy.state + DAG_ST_INC + gen, 1, dag_inc_patches(mb, sv.cells), ctl);
    return true;
}

// SOLVE = DAG_SOLVE_ALL: the launch also runs the systems' solve tasks (oisat_batch_analyse); the workgroup's LDS then also
// serves a sweep row's 128 x 129 block image + vectors (68 KB instead of 64: still two workgroups per CU).
// SOLVE = DAG_SOLVE_FWD: ONE system, and of its solve only the rows of the first forward sweep (dag_fwd_row_task) -- an
// instantiation of its own because the residual and increment bodies cost the K-loop its registers (DAG_SOLVE_ALL: 256 VGPRs
// and spills, this one none).  Its workgroups leave when the tickets are gone, except the first kDagFwdStayers, which serve
// the rows the chain still pushes: a few hundred idle workgroups polling the queue's counters would be memory-side traffic in
// the way of the chain's own polls, and one row per ~100 us of chain step needs a handful of workgroups.
constexpr int DAG_SOLVE_NONE = 0, DAG_SOLVE_ALL = 1, DAG_SOLVE_FWD = 2;
constexpr unsigned kDagFwdStayers = 16;
constexpr int kDagLdsFloats = 2 * 2 * NB * BK;                                  // the GEMM image, 65,536 B
constexpr int kDagSolveLdsFloats = NB * TLD + 4 * NB + 16;                      // block image | vec, part (doubles) | flag
static_assert(kDagSolveLdsFloats >= kDagLdsFloats && (size_t)kDagSolveLdsFloats * 4 >= 32768 + 2 * 1024 * sizeof(double) &&
              kSolveLdsBytes <= 32768, "solve tasks' LDS fits");
template <int SOLVE>
__global__ __launch_bounds__(256, 2) void potrf_dag_kernel(const DagSys* __restrict__ systems, const int4* __restrict__ tasks, int ntasks,
                                                           DagCtl* __restrict__ ctl, int* __restrict__ info, unsigned* __restrict__ err_total,
                                                           int* __restrict__ state_all, int state_words, int reserve_chains, int flags,
                                                           long long* __restrict__ trace, int chain_rows_total, const DagSolve sv) {
    __shared__ __attribute__((aligned(16))) float lds[SOLVE ? kDagSolveLdsFloats : kDagLdsFloats];
    __shared__ int s_ticket, s_flag, s_kav;
    static_assert(2 * D3_PBUF + 7 * D3_TILE + 2 * D3_TILE + 16 * D3_SLD <= 2 * 2 * NB * BK, "diagonal-block LDS fits into the GEMM image");
    const int t = threadIdx.x;
    DagLane L;                                                  // (dag_lane_coords, written out: through the call <1> spills 7 VGPRs more)
    L.lane = t & 63;
    L.wid = __builtin_amdgcn_readfirstlane(t >> 6);
    L.wr = L.wid >> 1;
    L.wc = L.wid & 1;
    L.rl = L.lane >> 3;
    L.lc = (L.lane & 7) ^ L.rl;
    L.frow = L.lane & 31;
    L.fh = L.lane >> 5;
    L.sw = L.frow & 7;
    L.arow = (L.wr * 64 + L.frow) * BK;
    L.brow = (L.wc * 64 + L.frow) * BK;
    L.flags = flags;
    L.spin = kDagSpinMax;
#ifdef OISAT_TEST_HOOKS
    if (flags & 256) L.spin = 4096u;
#endif
    // CU census (reserve_chains = number of leading chain tickets that want a CU to themselves): the first workgroup to start
    // on a CU draws its ticket and says what it drew; the second one waits for that word -- and for the chain tickets to be
    // gone, so that chains land on first arrivals -- and leaves at once if its CU belongs to a chain.  A chain alone on its
    // CU runs its diagonal blocks and 128^3 products at the rate of the stand-alone kernels (measured: 47 vs 60 us per block).
    int cu_key = -1, first_on_cu = 1;
    if (reserve_chains > 0 || SOLVE == DAG_SOLVE_ALL) {         // (a solving launch wants to know first from second too: above dag_queue_of)
        if (t == 0) {
            unsigned xcc, hw;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            const int key = (int)(((xcc & 15u) << 8) | ((hw >> 8) & 255u));
            const int arrived = __hip_atomic_fetch_add(&ctl->cu_arrivals[key], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_ticket = key;
            s_flag = arrived;
            if (arrived >= 1 && reserve_chains > 0) {           // bounded waits: a census that does not add up only costs the reservation
                unsigned spins = 0;
                while (__hip_atomic_load(&ctl->cu_role[key], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 && ++spins < 4096u)
                    __builtin_amdgcn_s_sleep(2);
                spins = 0;
                while (__hip_atomic_load(&ctl->ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < reserve_chains && ++spins < 4096u)
                    __builtin_amdgcn_s_sleep(2);
                s_kav = __hip_atomic_load(&ctl->cu_role[key], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                s_kav = 0;
            }
        }
        __syncthreads();
        cu_key = s_ticket;
        first_on_cu = s_flag == 0;
    }
    const bool second_on_cu = !first_on_cu;                     // takes the long VALU tasks of queue 1 (its CU-mate draws tile tasks)
    bool leave_now = reserve_chains > 0 && !first_on_cu && s_kav == 2;
    __syncthreads();
    __shared__ int4 s_task;
    bool tickets_gone = false;                                  // (block-uniform)
    unsigned idle = 0;
    long long wg_claim = 0, wg_first = 0, wg_tasks = 0, wg_n = 0;      // (tracing: time spent claiming work, in tasks)
    long long wg_pop[3] = {0, 0, 0};
    while (!leave_now) {
        __syncthreads();
        if (t == 0) {
            const long long c0 = trace ? wall_clock64() : 0;
            if (trace && wg_first == 0) wg_first = c0;
            int slot = -1;
            s_flag = 0;
            // a ready sweep row first (short, and a chain of others waits for it); a residual block / increment patch if this
            // workgroup is its CU's second one, or once the tickets are gone; else a ticket
            // (DAG_SOLVE_FWD does not time its claims: the array behind that pointer would be its only scratch)
            if (SOLVE && (dag_queue_pop(sv, ctl, 0, &s_task, &slot, trace && SOLVE == DAG_SOLVE_ALL ? wg_pop : (long long*)nullptr) ||
                          (SOLVE == DAG_SOLVE_ALL && (second_on_cu || tickets_gone) && dag_queue_pop(sv, ctl, 1, &s_task, &slot, trace ? wg_pop : (long long*)nullptr)))) {
                s_flag = 1;
                s_ticket = ntasks + slot;                                // (its row of the trace)
            } else if (!tickets_gone) {
                s_ticket = __hip_atomic_fetch_add(&ctl->ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                s_ticket = ntasks;
            }
            if (trace) wg_claim += wall_clock64() - c0;
        }
        __syncthreads();
        const int tk = s_ticket;
        const bool ready_task = SOLVE && s_flag != 0;
        if (cu_key >= 0 && first_on_cu) {                       // first ticket of the first workgroup of this CU: say what it is
            if (t == 0)
                __hip_atomic_store(&ctl->cu_role[cu_key], !ready_task && tk < reserve_chains ? 2 : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            cu_key = -1;
        }
        if (!ready_task && tk >= ntasks) {
            if (!SOLVE) break;
            // the tickets are gone; ready tasks may still come (the last systems' solves): until every system is done
            if (SOLVE == DAG_SOLVE_FWD && blockIdx.x >= kDagFwdStayers) break;      // (the stayers, or a smaller grid's every workgroup, serve the rows)
            tickets_gone = true;
            __syncthreads();
            if (t == 0) {
                const bool done = __hip_atomic_fetch_add(&ctl->sys_done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= sv.nsys;
                bool bad = dag_ld(&ctl->error) != 0;
                if (!done && !bad && ++idle > L.spin) {
                    dag_st(&ctl->error, 1);
                    bad = true;
                }
                s_flag = done || bad ? 1 : 0;
            }
            __syncthreads();
            if (s_flag != 0) break;
            __builtin_amdgcn_s_sleep(SOLVE == DAG_SOLVE_FWD ? 64 : 8);
            continue;
        }
        idle = 0;
        int4 task = ready_task ? s_task : tasks[tk];            // (kind, system, i, j) -- the same in every lane: say so
        task.x = __builtin_amdgcn_readfirstlane(task.x);
        task.y = __builtin_amdgcn_readfirstlane(task.y);
        task.z = __builtin_amdgcn_readfirstlane(task.z);
        task.w = __builtin_amdgcn_readfirstlane(task.w);
        const DagSys sy = systems[task.y];
        // tracing (OISAT_DAG_TRACE): per ticket [claimed, finished, time polling, T_j seen]; rows ntasks .. of the ready tasks:
        // [claimed, finished, -, the task packed]; the chains' stamps follow
        long long* tr = trace ? trace + 4 * (int64_t)tk : nullptr;
        if (tr && t == 0) {
            tr[0] = wall_clock64();
            tr[2] = 0;
            tr[3] = ready_task ? ((long long)task.x | ((long long)task.w << 4) | ((long long)task.y << 8) | ((long long)task.z << 24)) : 0;
        }
        bool ok;
        if constexpr (SOLVE == DAG_SOLVE_FWD) {
            // the lane's GEMM coordinates are formed per task, from a lane number the compiler cannot see through: kept across
            // the loop they are a dozen registers live through a sweep row, which then spills
            int tt = t;
            asm volatile("" : "+v"(tt));
            dag_lane_coords(L, tt);
            if (ready_task) ok = dag_fwd_row_task(sy, task.z, sv, ctl, lds);
            else if ((task.x & 255) == DAG_CHAIN)
                ok = dag_chain_task<true>(sy, ctl, info, lds, L, &s_flag, trace ? trace + 4 * (int64_t)(ntasks + sv.qcap) + 8 * (int64_t)task.z : nullptr, &sv);
            else ok = dag_tile_task<true>(sy, task.x & 255, (task.x >> 8) & 1023, task.x >> 18, task.z, task.w, ctl, lds, L, &s_flag, &s_kav, tr);
        } else if (ready_task) {
            const SolveMember mb = sv.mem[task.y];
            if (task.x == DAG_FWD) ok = dag_sweep_task<0>(sy, mb, task.y, task.z, task.w, sv, ctl, lds, &s_kav, L.spin);
            else if (task.x == DAG_BWD) ok = dag_sweep_task<1>(sy, mb, task.y, task.z, task.w, sv, ctl, lds, &s_kav, L.spin);
            else if (task.x == DAG_RES) ok = dag_res_task(sy, mb, task.y, task.z, task.w, sv, ctl, info, lds, &s_kav, L.spin);
            else if (sv.dtype == OISAT_F32) ok = dag_inc_task<float>(sy, mb, task.z, task.w, sv, ctl, lds);
            else ok = dag_inc_task<double>(sy, mb, task.z, task.w, sv, ctl, lds);
        } else if ((task.x & 255) == DAG_CHAIN) {
            ok = dag_chain_task<SOLVE != DAG_SOLVE_ALL>(sy, ctl, info, lds, L, &s_flag, trace ? trace + 4 * (int64_t)(ntasks + (SOLVE ? sv.qcap : 0)) + 8 * (int64_t)task.z : nullptr,
                                SOLVE ? &sv : (const DagSolve*)nullptr);
        } else {
            ok = dag_tile_task<SOLVE != DAG_SOLVE_ALL>(sy, task.x & 255, (task.x >> 8) & 1023, task.x >> 18, task.z, task.w, ctl, lds, L, &s_flag,
                                                       &s_kav, tr);                                          // (kind | k0 << 8 | kfar << 18)
        }
        if (tr && t == 0) {
            tr[1] = wall_clock64();
            wg_tasks += tr[1] - tr[0];
            ++wg_n;
        }
        if (!ok) break;
    }
    if (trace && t == 0) {                                      // per workgroup: [first claim, time claiming, time in tasks, tasks | left at]
        long long* w = trace + 4 * (int64_t)(ntasks + (SOLVE ? sv.qcap : 0)) + 8 * (int64_t)chain_rows_total + 8 * (int64_t)blockIdx.x;
        w[0] = wg_first; w[1] = wg_claim; w[2] = wg_tasks; w[3] = wg_n; w[4] = wall_clock64(); w[5] = 0; w[6] = wg_pop[0] + wg_pop[1]; w[7] = wg_pop[2];
    }
    // leave: the last workgroup out hands the progress words and the control block back clean
    __syncthreads();
    if (t == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this workgroup's last publish is acknowledged before it counts as gone
        const int gone = __hip_atomic_fetch_add(&ctl->gone, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_flag = gone == (int)gridDim.x - 1 ? 1 : 0;
    }
    __syncthreads();
    if (s_flag) {
        for (int w = t; w < state_words; w += 256) __hip_atomic_store(&state_all[w], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (reserve_chains > 0 || SOLVE == DAG_SOLVE_ALL)
            for (int w = t; w < DAG_CU_KEYS; w += 256) {
                __hip_atomic_store(&ctl->cu_arrivals[w], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&ctl->cu_role[w], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        if (SOLVE) {                                            // the ready queues' entries read "not written yet" again
            for (int w = t; w < 2 * sv.qcap; w += 256) __hip_atomic_store(&sv.queue[w], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (t == 0) {
            if (__hip_atomic_load(&ctl->error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) atomicAdd(err_total, 1u);
            for (int qi = 0; qi < 2; ++qi) {
                __hip_atomic_store(&ctl->q[qi].head, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&ctl->q[qi].tail, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&ctl->q[qi].avail, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __hip_atomic_store(&ctl->sys_done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&ctl->ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&ctl->error, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&ctl->gone, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
#undef DAG_MFMA4                                                // (defined in dense_kloop.inc for dag_seg; dag_self_product above is their other user)
#undef DAG_MFMA16

