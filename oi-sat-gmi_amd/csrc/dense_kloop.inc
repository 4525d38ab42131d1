// The fp32 K-loop of the 128x128 tile GEMM as a function over a K-segment, for the task-graph launch (dense_dag.inc).
// gemm_nt_big_kernel keeps its own copy of the loop (OISAT_DMA / OISAT_FRAG / OISAT_MFMA16): calling dag_seg there measured
// +2.5 % at K = 2048 (profiles/EXPERIMENTS.md, "One low-precision K-segment").  The image layout is the same in both.
// (Included by dense_dag.hip alone, inside its anonymous namespace; expects dense_tile.inc before it.)

struct DagLane {                 // a thread's fixed coordinates in the 128x128 tile GEMM
    int lane, wid, wr, wc, rl, lc, frow, fh, sw, arow, brow;
    int flags;                   // 0 in the product.  Only the -DOISAT_TEST_HOOKS build of the library (liboisat_hip_testhooks.so, loaded
                                 // by tests/test_gpu_dag.py alone) reads OISAT_DAG_FLAGS: 128 = fault injection -- no chain announces a
                                 // diagonal block from block 3 on (the waiters time out); 256 = polls give up after 4096 spins;
                                 // 512 = every chain step sleeps ~5 us (tools/chain_sensitivity.py)
    unsigned spin;               // polls before a wait gives up (kDagSpinMax)
};

// (flags and spin are the task-graph launch's own: it sets them)
__device__ __forceinline__ void dag_lane_coords(DagLane& L, int t) {
    L.lane = t & 63;
    L.wid = __builtin_amdgcn_readfirstlane(t >> 6);
    L.wr = L.wid >> 1;
    L.wc = L.wid & 1;
    // DMA: lane l lands at physical chunk (l & 7) of row (l >> 3) of its wave's piece, so it fetches the LOGICAL chunk lc
    L.rl = L.lane >> 3;
    L.lc = (L.lane & 7) ^ L.rl;
    // a lane's fragment of K-group s is logical chunk 2s+fh of its row: physical chunk (2s+fh) ^ (row&7).  Any 8 consecutive
    // rows hold one logical chunk in 8 different physical chunks = all 32 banks once: conflict-free ds_read_b128.
    L.frow = L.lane & 31;
    L.fh = L.lane >> 5;
    L.sw = L.frow & 7;
    L.arow = (L.wr * 64 + L.frow) * BK;
    L.brow = (L.wc * 64 + L.frow) * BK;
}

// lane's DMA source of operand tile `tile0` (a 128-row tile starting at row-major address tile0, leading dimension ld)
__device__ __forceinline__ const float* dag_src(const float* tile0, int64_t ld, const DagLane& L) {
    return tile0 + (int64_t)(L.wid * 32 + L.rl) * ld + 4 * L.lc;
}

// LDS-DMA (global_load_lds_dwordx4) of one K-step into buffer `buf` of the image lds = [buf][A|B][128 rows x 128 bytes]: wave
// `wid` brings rows wid*32 + 8i .. +7 (i = 0..3) of each operand, one KiB per instruction, straight into LDS -- no staging
// registers, no ds_write, and the wave only waits for its pieces right before the barrier.  A DMA instruction fills LDS
// linearly (lane l -> 16 bytes at 16 l), so the image cannot be padded; it is XOR-swizzled instead: every lane gives the
// source of the logical chunk that belongs at its physical place (DagLane::lc; still one 128-byte segment per row).
// a / b: this lane's source in row wid*32 + rl of each operand; sa / sb: bytes between the operand's rows (4 ld of an fp32
// matrix, 128 in a shadow tile).
__device__ __forceinline__ void dag_dma(float* __restrict__ lds, int buf, const DagLane& L, const char* a, int64_t sa, const char* b, int64_t sb) {
    typedef __attribute__((address_space(1))) const void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    constexpr int IMG = NB * BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        __builtin_amdgcn_global_load_lds((gptr_t)(a + 8 * i * sa), (lptr_t)(lds + (buf * 2 + 0) * IMG + (L.wid * 32 + 8 * i) * BK), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((gptr_t)(b + 8 * i * sb), (lptr_t)(lds + (buf * 2 + 1) * IMG + (L.wid * 32 + 8 * i) * BK), 16, 0, 0);
    }
}

// (also used by dag_self_product in dense_dag.inc, which #undef's both behind its kernel)
#define DAG_MFMA4(A0, A1, B0, B1, c)                                                            \
    acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(A0.c, B0.c, acc00, 0, 0, 0);                   \
    acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(A0.c, B1.c, acc01, 0, 0, 0);                   \
    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(A1.c, B0.c, acc10, 0, 0, 0);                   \
    acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(A1.c, B1.c, acc11, 0, 0, 0);
#define DAG_MFMA16(A0, A1, B0, B1)                                                              \
    DAG_MFMA4(A0, A1, B0, B1, x) DAG_MFMA4(A0, A1, B0, B1, y) DAG_MFMA4(A0, A1, B0, B1, z) DAG_MFMA4(A0, A1, B0, B1, w)

// acc += A[128 x 32 nkt] * B[128 x 32 nkt]^T over a K-segment: double-buffered LDS-DMA image, two fragment register sets --
// the operands of MFMA group s+1 are read from LDS while group s runs --, one barrier per K-step.  Ad / Bd: this lane's DMA
// source (dag_src) at the segment's first column.  On entry no wave reads or fills the LDS image; the same holds on return.
__device__ __forceinline__ void dag_seg(float* __restrict__ lds, const DagLane& L, const float* Ad, int64_t lda, const float* Bd, int64_t ldb,
                                        int nkt, f32x16& acc00, f32x16& acc01, f32x16& acc10, f32x16& acc11) {
    constexpr int IMG = NB * BK;                                // one operand image; lds = [buf][A|B][IMG]
#define DAG_DMA(buf, k0) dag_dma(lds, buf, L, (const char*)(Ad + (k0)), 4 * lda, (const char*)(Bd + (k0)), 4 * ldb)
#define DAG_FRAG(A0, A1, B0, B1, buf, s)                                                                               \
    do {                                                                                                           \
        A0 = *reinterpret_cast<const float4*>(lds + ((buf) * 2 + 0) * IMG + L.arow + 4 * ((2 * (s) + L.fh) ^ L.sw));            \
        A1 = *reinterpret_cast<const float4*>(lds + ((buf) * 2 + 0) * IMG + L.arow + 32 * BK + 4 * ((2 * (s) + L.fh) ^ L.sw));  \
        B0 = *reinterpret_cast<const float4*>(lds + ((buf) * 2 + 1) * IMG + L.brow + 4 * ((2 * (s) + L.fh) ^ L.sw));            \
        B1 = *reinterpret_cast<const float4*>(lds + ((buf) * 2 + 1) * IMG + L.brow + 32 * BK + 4 * ((2 * (s) + L.fh) ^ L.sw));  \
    } while (0)
    float4 fa0, fa1, fb0, fb1, ga0, ga1, gb0, gb1;
    DAG_DMA(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    DAG_FRAG(fa0, fa1, fb0, fb1, 0, 0);
    for (int kt = 0; kt < nkt; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nkt;
        if (more) DAG_DMA(cur ^ 1, (kt + 1) * BK);              // the other buffer is free since the last barrier
        DAG_FRAG(ga0, ga1, gb0, gb1, cur, 1);
        DAG_MFMA16(fa0, fa1, fb0, fb1)                         // s = 0
        DAG_FRAG(fa0, fa1, fb0, fb1, cur, 2);
        DAG_MFMA16(ga0, ga1, gb0, gb1)                         // s = 1
        DAG_FRAG(ga0, ga1, gb0, gb1, cur, 3);
        DAG_MFMA16(fa0, fa1, fb0, fb1)                         // s = 2
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's DMA pieces of K-step kt+1 have landed ...
        __syncthreads();                                        // ... everyone else's too; every read of K-step kt has been issued
        if (more) DAG_FRAG(fa0, fa1, fb0, fb1, cur ^ 1, 0);     // first operands of the next K-step, behind the last MFMA group
        DAG_MFMA16(ga0, ga1, gb0, gb1)                         // s = 3
    }
#undef DAG_DMA
#undef DAG_FRAG
}
