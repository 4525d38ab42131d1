// The diagonal block's device functions: the 16x16 factorization in registers (diag16_*) and the waves of the register-resident
// 128x128 block (d3_*).  Included by dense_dag.hip alone, inside its anonymous namespace: potrf_diag3_kernel and the task-graph
// kernel's chains both run these waves, and the two kernels share a translation unit (profiles/EXPERIMENTS.md: alone,
// potrf_diag3_kernel compiles to other instructions).  Expects dense_tile.inc (NB) before it.
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Factor and invert a 16x16 diagonal block in ONE sweep, in registers.  Lane r of every 16-lane row holds row r of the
// block (d[c] = A[r][c]) and column r of the running inverse (x[c] = X[c][r], X = L^-1, starts as I): after pivot step k
// column k of L is final, which is exactly what the forward substitution for X needs next, so each broadcast
// L[c][k] = d[k] of lane c feeds both the factor's trailing update and the inverse's running sums.
// The broadcast is the DPP operand of the FMA itself (row_newbcast:c = lane c of each 16-lane row, gfx90a+):
//     d[c] += (-d[k] @ lane c) * d[k]        x[c] += (-d[k] @ lane c) * x[k]        (v_fmac_f32_dpp)
// two vector instructions per (k, c) and no scalar registers.  (Rounds 1-2 broadcast through v_readlane: 240 scalar
// values live across the unrolled sweep, which the compiler spilled to VGPR lanes with ~350 v_writelane / ~640
// v_readlane -- 310 cycles per pivot; the builtin DPP move is not folded into the FMA by the compiler either, hence
// the inline assembly.)  Hazard: a VGPR written by a VALU instruction may be read through DPP two wait states later at
// the earliest and the compiler does not see into the asm blocks -- diag16_settle() puts the s_nop between the
// instruction that finishes column k and its DPP readers, and every asm block here is volatile, i.e. stays in order.
template <int C>
__device__ __forceinline__ float row16_bcast_settled(float v) {          // v was last written by one of the asm blocks
    float o;
    asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(o) : "v"(v), "n"(C));
    return o;
}

__device__ __forceinline__ void diag16_settle(float& dk, float& xk) {
    asm volatile("s_nop 1" : "+v"(dk), "+v"(xk));
}

template <int K, int C, int CEND>            // columns C .. CEND-1 receive pivot K's update
__device__ __forceinline__ void diag16_columns(float (&d)[16], float (&x)[16]) {
    if constexpr (C < CEND) {
        asm volatile("v_fmac_f32_dpp %0, -%2, %2 row_newbcast:%4 row_mask:0xf bank_mask:0xf\n\t"
                     "v_fmac_f32_dpp %1, -%2, %3 row_newbcast:%4 row_mask:0xf bank_mask:0xf"
                     : "+v"(d[C]), "+v"(x[C]) : "v"(d[K]), "v"(x[K]), "n"(C));
        diag16_columns<K, C + 1, CEND>(d, x);
    }
}

// pivot K: broadcast, reciprocal square root (+ one Newton step), scale column K of L and row K of X.  Plain C between
// the asm blocks: the compiler is free to spread these dependent instructions among the (independent) FMAs of the
// previous pivot that follow in program order.
template <int K>
__device__ __forceinline__ void diag16_pivot(float (&d)[16], float (&x)[16], int r, int& bad) {
    float piv = row16_bcast_settled<K>(d[K]);
    const bool neg = !(piv > 0.f);
    bad = (neg && bad == 0) ? K + 1 : bad;
    piv = neg ? 1.f : piv;
    float ri = __builtin_amdgcn_rsqf(piv);
    ri = ri * (1.5f - 0.5f * piv * ri * ri);              // one Newton step: ~0.5 ulp
    d[K] = (r == K) ? piv * ri : d[K] * ri;               // L[k][k] = sqrt(piv); column k of L
    x[K] = (K >= r) ? x[K] * ri : 0.f;                    // X[k][:] /= L[k][k]
}

// Software-pipelined sweep: as soon as column K+1 has received pivot K's update, pivot K+1's dependent chain
// (broadcast -> rsq -> Newton -> scale) is started, and the remaining updates of pivot K (columns K+2..15, independent
// of it) fill its latency.  Same arithmetic in the same order as the plain sweep.
template <int K>
__device__ __forceinline__ void diag16_pivots(float (&d)[16], float (&x)[16], int r, int& bad) {
    if constexpr (K == 0) diag16_pivot<0>(d, x, r, bad);
    if constexpr (K < 15) {
        diag16_settle(d[K], x[K]);
        diag16_columns<K, K + 1, K + 2>(d, x);             // column K+1 is final
        diag16_pivot<K + 1>(d, x, r, bad);
        diag16_columns<K, K + 2, 16>(d, x);
        diag16_pivots<K + 1>(d, x, r, bad);
    }
}

__device__ __forceinline__ void diag16_report(int bad, int* info, int col0, int lane, int which) {
    if (bad && lane == 0) {               // info[0]: this factorization; info[1], info[2]: sticky (first column, count)
        atomicCAS(info, 0, col0 + bad);  //          until oisat_solve_status clears them
        atomicCAS(info + 1, 0, col0 + bad);
        atomicAdd(info + 2, 1);
        atomicCAS(info + 3, 0, which + 1);             // batched factorization: which matrix of the table (1-based)
    }
}

// ---- diagonal block, REGISTER-RESIDENT: Cholesky + inverse of one 128x128 block, one workgroup of 4 waves, 24 KB of LDS ------
// The 36 lower 16x16 tiles of the block live in MFMA accumulator registers for the whole kernel: the 8 diagonal tiles in
// wave 0 (which also runs the serial 16x16 factorizations), off-diagonal tile (I, K), idx = I(I-1)/2 + K, in wave
// 1 + idx % 3, slot idx / 3 (10 / 9 / 9 tiles).  A slot's accumulator holds A[I,K] until its panel step K makes it the
// final L[I,K]; from then on the SAME register accumulates the running inverse X[I,K] until step I finishes it.  The
// A phase holds the tile TRANSPOSED (lane: A[lr][4 lg + e], one float4 of a row): the trailing update just swaps its two
// operands, and the panel product P_I^T = Dinv_J * A[I,J]^T then takes the held tile straight from the registers as the
// MFMA's B operand (d3_mma_regb) -- as does X[J,K] = Dinv_J * accX[J,K] -- so the workers never stage a tile.  Every
// tile coordinate is a compile-time constant of the wave's code path (one instantiation per wave), so each wave
// executes straight-line code with exactly its own tile operations.  LDS only
// carries what other waves need as MFMA operands: the current panel column P (= final L[:, J]), row J of X = L^-1, the
// inverse of the current diagonal 16x16 block, and one staging tile for the 16x16 factorization (accumulator layout ->
// lane = row).  Right-looking at 16-column granularity, per block column J:
//   (1) the wave that owns tile (J, J) factors and inverts it in registers (diag16_pivots: lane = row);
//   (2) panel:      P_I = A[I,J] * Dinv_J^T  (I > J)           row J of X:  X[J,K] = Dinv_J * accX[J,K]  (K < J)
//   (3) trailing:   A[I,K] -= P_I * P_K^T  (I >= K > J)        inverse:     accX[I,K] -= P_I * X[J,K]    (I > J >= K)
// i.e. the forward substitution for X = L^-1 rides along with the factorization (row J of X is final as soon as Dinv_J
// is) instead of a separate doubling phase, the trailing updates never move an accumulator through LDS, and the owner
// of (J+1, J+1) updates that tile first and factors it while the other waves finish step J (look-ahead).
typedef __attribute__((address_space(1))) float gfloat;          // global address space: global_load / global_store, which the
typedef __attribute__((address_space(1))) f32x4 gf32x4;         // LDS-only barrier does not wait for (flat_* count on lgkmcnt too)
constexpr int D3_WAVES = 4, D3_THREADS = 64 * D3_WAVES, D3_LD = 17, D3_TILE = 16 * D3_LD, D3_PBUF = 7 * D3_TILE;

constexpr int d3_I(int idx) {              // idx = I(I-1)/2 + K, 0 <= K < I < 8
    int I = 1;
    while (I * (I + 1) / 2 <= idx) ++I;
    return I;
}
constexpr int d3_K(int idx) { return idx - d3_I(idx) * (d3_I(idx) - 1) / 2; }

// acc (rows 4*lg + e, column lr) += sum_k (+-a[lr][k]) * B[k][lr-th column]: 4 MFMAs over k = 4s + lg
// A operand: element [lr][4s + lg] of a row-major 16 x D3_LD tile (negated if NEG); B operand either
//   BT = true:  B[k][col] = bt[col][k]  -> element [lr][4s + lg] of bt           (C -= A * B^T form)
//   BT = false: B[k][col] = b[k][col]   -> element [4s + lg][lr] of b
template <bool NEG, bool BT>
__device__ __forceinline__ f32x4 d3_mma(f32x4 acc, const float* a, const float* b, int lr, int lg) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float av = a[lr * D3_LD + 4 * s + lg];
        const float bv = BT ? b[lr * D3_LD + 4 * s + lg] : b[(4 * s + lg) * D3_LD + lr];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(NEG ? -av : av, bv, acc, 0, 0, 0);
    }
    return acc;
}

// D = a * R with R held in accumulator layout by the calling wave (lane: R[4 lg + e][lr]): the MFMA's k index is only a
// summation index, so step s takes k = 4 lg + s -- B operand = the lane's own breg[s], A operand = a[lr][4 lg + s].
// No staging through LDS.
__device__ __forceinline__ f32x4 d3_mma_regb(const float* a, f32x4 breg, int lr, int lg) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[lr * D3_LD + 4 * lg + s], breg[s], acc, 0, 0, 0);
    return acc;
}

// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for the wave's outstanding GLOBAL stores
// (vmcnt(0)) -- here the final L and T tiles stream out to HBM in every step and nobody in the workgroup reads them back,
// so waiting for their acknowledgement (1-2 us each time) is pure loss.
__device__ __forceinline__ void d3_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Global stores of the diagonal-block kernel: (wave-uniform base, per-lane element offset).  WT (the task-graph factorization,
// where OTHER workgroups of the same launch read L and T): write-through `sc1` stores -- the bytes leave the XCD's L2 at once,
// so publishing them takes a drained vmcnt and a flag instead of an L2 write-back (buffer_wbl2) per diagonal block.  Buffer
// stores, not inline assembly: the stored values come straight out of MFMA instructions, and the wait states between an MFMA
// and a memory instruction that reads its result are the compiler's to insert -- it does not look into asm blocks (a
// global_store in inline assembly stored the register's OLD content: one wrong element per tile, found the hard way).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t d3_rsrc(const gfloat* base) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, 0x7ffffff0, 0x00020000);
}
template <bool WT>
__device__ __forceinline__ void d3_gst(gfloat* base, int64_t off, float v) {
    if (WT) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), d3_rsrc(base), (int)(off * 4), 0, 16);
    else base[off] = v;
}
template <bool WT>
__device__ __forceinline__ void d3_gst4(gfloat* base, int64_t off, f32x4 v) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    if (WT) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), d3_rsrc(base), (int)(off * 4), 0, 16);
    else *reinterpret_cast<gf32x4*>(base + off) = v;
}

// Loads of the block's tiles.  WT: `sc1` buffer loads (served by L2, never by this CU's L1, which may hold the tile as it was
// before another workgroup -- or this one's write-through stores -- updated it).
template <bool WT>
__device__ __forceinline__ float d3_gld(const gfloat* Sb, int64_t ld, int row, int col) {
    if (WT) {
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(d3_rsrc(Sb), (int)((row * ld + col) * 4), 0, 16));
    }
    return Sb[(int64_t)row * ld + col];
}
template <bool WT>
__device__ __forceinline__ f32x4 d3_gld4(const gfloat* Sb, int64_t ld, int row, int col) {
    if (WT) {
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(d3_rsrc(Sb), (int)((row * ld + col) * 4), 0, 16));
    }
    return *reinterpret_cast<const gf32x4*>(Sb + (int64_t)row * ld + col);
}

__device__ __forceinline__ void d3_put(float* tile, f32x4 acc, int lr, int lg) {   // accumulator layout -> row-major tile
#pragma unroll
    for (int e = 0; e < 4; ++e) tile[(4 * lg + e) * D3_LD + lr] = acc[e];
}

// factor + invert the diagonal tile held in `acc` (by the calling wave): L16 (full rows, the upper part is garbage) to
// `stage`, X16 = L16^-1 to `dinv`; a worker wave copies both to global memory in the next panel phase
constexpr int D3_SLD = 20;                 // row stride of the staging tile: 16-byte aligned rows (ds_read_b128 / ds_write_b128)
__device__ __forceinline__ void d3_diag16(f32x4 acc, float* stage, float* dinv, int* info, int col0, int lane, int lr, int lg, int which) {
#pragma unroll
    for (int e = 0; e < 4; ++e) stage[(4 * lg + e) * D3_SLD + lr] = acc[e];
    __builtin_amdgcn_wave_barrier();
    float d[16], x[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(stage + lr * D3_SLD + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) d[4 * q + e] = v[e];
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) x[c] = (c == lr) ? 1.f : 0.f;
    int bad = 0;
    diag16_pivots<0>(d, x, lr, bad);
    diag16_report(bad, info, col0, lane, which);
    __builtin_amdgcn_wave_barrier();
    if (lane < 16) {                       // (the other three 16-lane rows hold copies)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<f32x4*>(stage + lr * D3_SLD + 4 * q) = f32x4{d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]};   // L16[lr][:]
#pragma unroll
        for (int c = 0; c < 16; ++c) dinv[c * D3_LD + lr] = x[c];                                                             // X16[c][lr]
    }
}

// a worker copies the freshly factored diagonal tile J to global memory: L16 (lower part) and T's diagonal tile
template <bool WT>
__device__ __forceinline__ void d3_store_diag(gfloat* Sjj, int64_t ld, gfloat* Tjj, const float* stage, const float* dinv, int lr, int lg) {
    const f32x4 l = *reinterpret_cast<const f32x4*>(stage + lr * D3_SLD + 4 * lg);
    f32x4 t;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        t[e] = dinv[lr * D3_LD + 4 * lg + e];
        if (4 * lg + e <= lr) d3_gst<WT>(Sjj, (int64_t)lr * ld + 4 * lg + e, l[e]);
    }
    d3_gst4<WT>(Tjj, lr * NB + 4 * lg, t);
}

// wave 0: the diagonal tiles
template <bool WT>
__device__ __forceinline__ void d3_diagonal_wave(gfloat* Sb, int64_t ld, const float* Pp, float* dinvb, float* stage, int* info,
                                                 int col0, int lane, int lr, int lg, int which) {
    f32x4 accD[8];
#pragma unroll
    for (int J = 0; J < 8; ++J)
#pragma unroll
        for (int e = 0; e < 4; ++e) accD[J][e] = d3_gld<WT>(Sb, ld, 16 * J + 4 * lg + e, 16 * J + lr);
    d3_diag16(accD[0], stage, dinvb, info, col0, lane, lr, lg, which);
#pragma unroll
    for (int J = 0; J < 8; ++J) {
        d3_barrier();                      // Dinv_J is in LDS; every wave is done with step J-1
        if (J >= 1) {                      // while the workers build panel J: the later diagonal tiles catch up with panel J-1
            const float* pp = Pp + ((J - 1) & 1) * D3_PBUF;
#pragma unroll
            for (int K = J + 1; K < 8; ++K) accD[K] = d3_mma<true, true>(accD[K], pp + (K - 1) * D3_TILE, pp + (K - 1) * D3_TILE, lr, lg);
        }
        d3_barrier();                      // the panel and row J of X are in LDS
        if (J == 7) break;
        // look-ahead: tile (J+1, J+1) takes panel J's update and is factored at once (its older updates are in already)
        const float* pj = Pp + (J & 1) * D3_PBUF + J * D3_TILE;
        accD[J + 1] = d3_mma<true, true>(accD[J + 1], pj, pj, lr, lg);
        d3_diag16(accD[J + 1], stage, dinvb + ((J + 1) & 1) * D3_TILE, info, col0 + 16 * (J + 1), lane, lr, lg, which);
    }
}

// waves 1..3: the off-diagonal tiles idx = 3 t + W - 1
template <int W, bool WT>
__device__ __forceinline__ void d3_worker_wave(gfloat* Sb, int64_t ld, gfloat* Tg, float* Pp, float* Xr, const float* dinvb, const float* stage,
                                               int lr, int lg) {
    constexpr int NS = (28 - (W - 1) + 2) / 3;
    f32x4 acc[NS];
#pragma unroll
    for (int t = 0; t < NS; ++t) {
        const int I = d3_I(3 * t + W - 1), K = d3_K(3 * t + W - 1);
        acc[t] = d3_gld4<WT>(Sb, ld, 16 * I + lr, 16 * K + 4 * lg);                                             // A[I,K]^T
        d3_gst4<WT>(Tg, (16 * K + lr) * NB + 16 * I + 4 * lg, f32x4{0.f, 0.f, 0.f, 0.f});                         // T is lower triangular
    }
#pragma unroll
    for (int J = 0; J < 8; ++J) {
        const float* dinv = dinvb + (J & 1) * D3_TILE;
        float* P = Pp + (J & 1) * D3_PBUF;                 // panel J: tile I (>= 1) at P + (I - 1) * D3_TILE; two buffers, by parity of J
        d3_barrier();                      // Dinv_J is in LDS; every wave is done with step J-1 (P, Xr may be rewritten)
        if (J % 3 == W - 1)                // the diagonal tile wave 0 has just factored: to global memory
            d3_store_diag<WT>(Sb + (int64_t)16 * J * ld + 16 * J, ld, Tg + 16 * J * NB + 16 * J, stage, dinv, lr, lg);
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const int I = d3_I(3 * t + W - 1), K = d3_K(3 * t + W - 1);
            if (K == J) {                  // panel tile: P_I^T = Dinv_J * A[I,J]^T, P_I = final L[I,J]; the slot turns to X[I,J]
                const f32x4 pt = d3_mma_regb(dinv, acc[t], lr, lg);             // lane: P_I[lr][4 lg + e]
#pragma unroll
                for (int e = 0; e < 4; ++e) P[(I - 1) * D3_TILE + lr * D3_LD + 4 * lg + e] = pt[e];
                d3_gst4<WT>(Sb, (int64_t)(16 * I + lr) * ld + 16 * J + 4 * lg, pt);
                acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            } else if (I == J) {           // row J of the inverse (K < J): X[J,K] = Dinv_J * acc
                const f32x4 xf = d3_mma_regb(dinv, acc[t], lr, lg);
                d3_put(Xr + K * D3_TILE, xf, lr, lg);
#pragma unroll
                for (int e = 0; e < 4; ++e) d3_gst<WT>(Tg, (16 * J + 4 * lg + e) * NB + 16 * K + lr, xf[e]);
            }
        }
        d3_barrier();                      // the panel and row J of X are in LDS
        if (J == 7) break;
#pragma unroll
        for (int t = 0; t < NS; ++t) {
            const int I = d3_I(3 * t + W - 1), K = d3_K(3 * t + W - 1);
            if (I > J) {
                if (K > J) acc[t] = d3_mma<true, true>(acc[t], P + (K - 1) * D3_TILE, P + (I - 1) * D3_TILE, lr, lg);          // A[I,K]^T -= P_K P_I^T
                else acc[t] = d3_mma<true, false>(acc[t], P + (I - 1) * D3_TILE, K == J ? dinv : Xr + K * D3_TILE, lr, lg);   // X[I,K] -= L[I,J] X[J,K]
            }
        }
    }
}
