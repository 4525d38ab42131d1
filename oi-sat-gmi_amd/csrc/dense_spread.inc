// The spread of a panel of vectors over the cells, shared by the randomized error (dense_cov.hip: oisat_probe_spread, MEMBER =
// false) and the posterior ensemble (dense_ensemble.hip: oisat_member_spread, MEMBER = true).  Included inside the anonymous
// namespace of both units, behind dense_solve_dev.inc (latitude window, block_sphere, corr_f32).
//
// ---- probe spread: t_ik = sig_i sum_a C(i,a) osig_a U[k][a] for a group of G probes at once --------------------------------
// The increment with K vectors in the place of z: thread = one cell (a 32 x 8 patch of the grid, or 256 consecutive cells), the
// increment's latitude window and bounding-sphere cull (block_sphere), the surviving observations staged in LDS as double
// coordinates + index.  Per group of G probes the staged observations pass in sub-chunks of 64 whose weights osig_a U[k][a]
// are gathered into LDS ([64][G], read back as wave-uniform 16-byte words), so that one evaluation of the correlation --
// |p - q|^2 in double from the double coordinates, corr_f32 -- serves G fused multiply-adds into G fp32 sums.  The squares and
// fourth powers of sig_i t_ik are added in double at the end of the group.  The group loop is the outer one (the sums of
// one group live in registers across the whole candidate range), so a pair's correlation is evaluated nprobe / G times.
// Fixed order everywhere: candidate order, then k.  No far tier.
// MEMBER: the sum is not squared but taken off a stored row, P[k][i] <- (float)(P[k][i] - sig_i t_ik) in double with one
// rounding, and the squares and fourth powers are those of the value stored.  Everything ahead of a group's end is the same
// code, so the sums t_ik have the bits of the probe spread.
constexpr int kSpreadStage = 512;                              // staged observations: processed once 256 have gathered
constexpr int kSpreadSub = 64;                                 // observations per weight image
template <int KIND, int G, bool MEMBER>
__global__ __launch_bounds__(256) void probe_spread_kernel(const double* __restrict__ gxyz, const double* __restrict__ gsig, int64_t n, int nx,
                                                            const double* __restrict__ oxyz, const double* __restrict__ osig,
                                                            const float* __restrict__ U, int nprobe, int64_t ldu, int64_t m, float g2,
                                                            const double* __restrict__ glat, const double* __restrict__ olat, double win_deg,
                                                            double cut_chord, int accumulate, double* __restrict__ sum2,
                                                            double* __restrict__ sum4, float* __restrict__ P, int64_t ldp) {
    constexpr int GS = G + 4;                                   // row stride of the weight image (16-byte aligned rows)
    __shared__ double sx[kSpreadStage], sy[kSpreadStage], sz[kSpreadStage];
    __shared__ int sidx[kSpreadStage];
    __shared__ __attribute__((aligned(16))) float sw[kSpreadSub * GS];
    __shared__ double red[16], s_lo[4], s_hi[4];
    __shared__ int64_t s_j[2];
    __shared__ int wcnt[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t blk = blockIdx.x;
    int64_t cell;
    bool live;
    if (nx > 0) {                                               // patch `blk` of the ny x nx grid
        const int64_t ny = n / nx, ppr = (nx + 31) / 32;
        const int64_t yy = (blk / ppr) * 8 + (t >> 5), xx = (blk % ppr) * 32 + (t & 31);
        live = yy < ny && xx < nx;
        cell = yy * nx + xx;
    } else {
        cell = blk * 256 + t;
        live = cell < n;
    }
    const double px[1] = {live ? gxyz[cell] : 0.0}, py[1] = {live ? gxyz[n + cell] : 0.0}, pz[1] = {live ? gxyz[2 * n + cell] : 0.0};
    const bool lv[1] = {live};
    int64_t j0 = 0, j1 = m;
    const bool windowed = glat && olat;
    if (windowed) {                                             // latitude span of this block's cells -> observation index range
        double lo = live ? glat[cell] : 1e9, hi = live ? glat[cell] : -1e9;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o, kWave)); hi = fmax(hi, __shfl_xor(hi, o, kWave)); }
        if (lane == 0) { s_lo[w] = lo; s_hi[w] = hi; }
        __syncthreads();
        if (t == 0) {
            lo = fmin(fmin(s_lo[0], s_lo[1]), fmin(s_lo[2], s_lo[3]));
            hi = fmax(fmax(s_hi[0], s_hi[1]), fmax(s_hi[2], s_hi[3]));
            s_j[0] = lower_bound_lat(olat, m, lo - win_deg);
            s_j[1] = lower_bound_lat(olat, m, hi + win_deg + 1e-9);
        }
        __syncthreads();
        j0 = s_j[0];
        j1 = s_j[1];
    }
    const BlockSphere bs = block_sphere<1>(px, py, pz, lv, windowed ? cut_chord : 1e30, (double)INFINITY, red);
    const double sg = live ? gsig[cell] : 0.0;
    double s2 = 0.0, s4 = 0.0;
    for (int k0 = 0; k0 < nprobe; k0 += G) {
        float acc[G];
#pragma unroll
        for (int kk = 0; kk < G; ++kk) acc[kk] = 0.f;
        int fill = 0;
        for (int64_t c0 = j0; c0 < j1; c0 += 256) {
            {   // one pass of 256 candidates: the survivors of the cull go to the stage in candidate order
                const int64_t c = c0 + t;
                double x = 0.0, y = 0.0, zz = 0.0;
                bool keep = false;
                if (c < j1) {
                    x = oxyz[c]; y = oxyz[m + c]; zz = oxyz[2 * m + c];
                    const double dx = x - bs.cx, dy = y - bs.cy, dz = zz - bs.cz;
                    keep = dx * dx + dy * dy + dz * dz <= bs.r2cull;
                }
                const unsigned long long mask = __ballot(keep);
                if (lane == 0) wcnt[w] = __popcll(mask);
                __syncthreads();
                const int c0w = wcnt[0], c1w = wcnt[1], c2w = wcnt[2], c3w = wcnt[3];
                if (keep) {
                    const int pos = fill + (w > 0 ? c0w : 0) + (w > 1 ? c1w : 0) + (w > 2 ? c2w : 0) + __popcll(mask & ((1ull << lane) - 1ull));
                    sx[pos] = x; sy[pos] = y; sz[pos] = zz;
                    sidx[pos] = (int)c;
                }
                __syncthreads();
                fill += c0w + c1w + c2w + c3w;
            }
            if (fill < 256 && c0 + 256 < j1) continue;          // (block-uniform) at most 255 + 256 entries ever wait
            for (int s0 = 0; s0 < fill; s0 += kSpreadSub) {
                const int cnt = fill - s0 < kSpreadSub ? fill - s0 : kSpreadSub;
                if (lane < cnt) {                               // weights: wave w takes the probes w, w + 4, ..; a lane one observation
                    const int a = sidx[s0 + lane];
                    const float so = (float)osig[a];
                    for (int kk = w; kk < G; kk += 4) sw[lane * GS + kk] = so * U[(int64_t)(k0 + kk) * ldu + a];
                }
                __syncthreads();
                for (int o = 0; o < cnt; ++o) {
                    const double dx = px[0] - sx[s0 + o], dy = py[0] - sy[s0 + o], dz = pz[0] - sz[s0 + o];
                    const float c = corr_f32<KIND>(g2, (float)(dx * dx + dy * dy + dz * dz));
#pragma unroll
                    for (int kk = 0; kk < G; kk += 4) {
                        const float4 wv = *reinterpret_cast<const float4*>(&sw[o * GS + kk]);
                        acc[kk] = __builtin_fmaf(c, wv.x, acc[kk]);
                        acc[kk + 1] = __builtin_fmaf(c, wv.y, acc[kk + 1]);
                        acc[kk + 2] = __builtin_fmaf(c, wv.z, acc[kk + 2]);
                        acc[kk + 3] = __builtin_fmaf(c, wv.w, acc[kk + 3]);
                    }
                }
                __syncthreads();
            }
            fill = 0;
        }
        if (MEMBER) {
            if (live) {
#pragma unroll
                for (int kk = 0; kk < G; ++kk) {                // (a live thread's cell < n <= ldp; k0 + kk < nprobe rows of P)
                    float* __restrict__ pk = P + (int64_t)(k0 + kk) * ldp + cell;
                    const float v = (float)((double)*pk - sg * (double)acc[kk]);
                    *pk = v;
                    const double q = (double)v * (double)v;
                    s2 += q;
                    s4 += q * q;
                }
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < G; ++kk) {
                const double td = sg * (double)acc[kk], q = td * td;
                s2 += q;
                s4 += q * q;
            }
        }
    }
    if (live) {
        sum2[cell] = accumulate ? sum2[cell] + s2 : s2;
        sum4[cell] = accumulate ? sum4[cell] + s4 : s4;
    }
}

// The host side of both entry points: argument checks, the window, the grid.  nx = 0: ny consecutive cells.  Groups of 64
// vectors where nvec allows it (half the evaluations of a pair's correlation).
template <bool MEMBER>
static int spread_launch(oisat_ctx* h, const char* name, const double* gxyz, const double* gsig, int64_t ny, int64_t nx, const double* oxyz,
                         const double* osig, const float* U, int64_t nvec, int64_t ldu, int64_t m, double g, const double* glat,
                         const double* olat_sorted, int accumulate, double* sum2_out, double* sum4_out, float* P, int64_t ldp) {
    ARG_CHECK(h && gxyz && gsig && oxyz && osig && U && sum2_out && sum4_out && ny > 0 && m > 0 && m < (int64_t)INT32_MAX && g >= 0.0);
    ARG_CHECK(nx >= 0 && nx < (int64_t)INT32_MAX);
    ARG_CHECK(nvec >= 32 && nvec <= 4096 && nvec % 32 == 0 && ldu >= m);
    const int64_t n = nx > 0 ? ny * nx : ny;
    ARG_CHECK(!MEMBER || (P != nullptr && ldp >= n));
    const double win = lat_window_deg(h->corr, g);
    if (!(win < 180.0) || !glat || !olat_sorted) { glat = nullptr; olat_sorted = nullptr; }
    const int64_t gx = increment_blocks(n, nx, 1);
    ARG_CHECK(gx < (int64_t)INT32_MAX);
    const float g2 = (float)corr_scale2(h->corr, g);
    if (nvec % 64 == 0) {
        OISAT_LAUNCH_CORR(h, name, probe_spread_kernel, OISAT_TARGS(64, MEMBER), dim3((unsigned)gx), dim3(256), 0, gxyz, gsig, n, (int)nx, oxyz,
                          osig, U, (int)nvec, ldu, m, g2, glat, olat_sorted, win, cut_chord_of(h->corr, g), accumulate, sum2_out, sum4_out, P, ldp);
    } else {
        OISAT_LAUNCH_CORR(h, name, probe_spread_kernel, OISAT_TARGS(32, MEMBER), dim3((unsigned)gx), dim3(256), 0, gxyz, gsig, n, (int)nx, oxyz,
                          osig, U, (int)nvec, ldu, m, g2, glat, olat_sorted, win, cut_chord_of(h->corr, g), accumulate, sum2_out, sum4_out, P, ldp);
    }
    return OISAT_OK;
}
