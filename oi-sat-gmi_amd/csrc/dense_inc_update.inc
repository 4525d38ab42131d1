// The increment behind a correction as an UPDATE of the first solve's: fields = T(inc0 + delta), delta = sig_i sum_a C(i,a) sig_a (z - z0)_a.
// Device code of oisat_gain_solve_fields (dense_solve.hip; kernel and launches: dense_cov.hip), included inside dense_cov.hip's
// anonymous namespace behind dense_solve_dev.inc.
// The increment is linear in z.  inc0 = B H^T z0 is evaluated in float64 from the FIRST solve's z0 (apply_increment_kernel into a
// double scratch field, on the handle's side stream underneath the correction's sweeps); what the refinement adds to z0 is dz with
// |dz| ~ |r_0| / |d| of |z0| (2.4e-5 on the headline months), so its image on the grid needs four digits where inc0 needs sixteen:
// every pair is evaluated the way resid_update_block evaluates S dz -- fp32 coordinates, v_pk_* / v_exp_f32, fp32 partial sums
// joined in double.  The differences z - z0 are taken in DOUBLE while staging (they cancel to 1e-5 of either), the product with
// sig_i and the sum with inc0 are double, and each field is rounded to T once.
// Geometry: increment_patch's -- the same patches (CELLS * 8 rows x 32 columns), latitude window and bounding-sphere cull -- but the
// window and the cull are cut at 2^-kIncUpdateCutBits instead of 2^-52: a term below 2^-20 of a unit term changes delta by less than
// 1e-6 of itself (the protocol's months: about 0.4 of the increment's pairs).  Staging: resid_update_block's four float arrays
// x[] | y[] | z[] | w[] (w = sig dz) of kUpdStage entries in the bytes of bxy | bzw, padded with weight-0 entries to a multiple of 16,
// flushed once another pass of 256 candidates might not fit or behind the last pass -- a rule of the counts alone.  Every thread
// walks the whole list in quads (wave-uniform addresses: broadcast reads), entries (0, 1) and (2, 3) of a quad in the two lanes of two
// partial sums per cell; the partial sums join the cell's double sum every 64 entries (16 terms per lane), in a fixed order.
// skip_sums (block-uniform): the refinement converged at r_0, z = z0 -- nothing is summed and the fields are T(inc0), T(xb + inc0):
// the bits of the float64 increment of z0.
constexpr double kIncUpdateCutBits = 20.0;

template <typename T, int CELLS>
__device__ __forceinline__ void increment_update_patch(const double* __restrict__ gxyz, const double* __restrict__ gsig, int64_t n,
                                                       const double* __restrict__ oxyz, const double* __restrict__ osig,
                                                       const double* __restrict__ z, const double* __restrict__ z0, int64_t m, double g2,
                                                       const T* __restrict__ xb, T* __restrict__ xa, T* __restrict__ inc,
                                                       const double* __restrict__ inc0, const double* __restrict__ glat,
                                                       const double* __restrict__ olat, double win_deg, int nx, double cut_chord,
                                                       bool skip_sums, int64_t blk, const SolveLds& W) {
    static_assert(kUpdStage % 16 == 0 && kUpdStage >= 512, "the padded list must fit");
    constexpr int PW = 32, PH = CELLS * 8;
    float* const lx = (float*)W.bxy;                            // bxy and bzw are adjacent (solve_lds_carve)
    float* const ly = lx + kUpdStage;
    float* const lz = ly + kUpdStage;
    float* const lw = lz + kUpdStage;
    const int t = threadIdx.x;
    const int64_t ny = n / nx;
    const int64_t ppr = (nx + PW - 1) / PW;                     // patches per row of patches
    if (blk >= ppr * ((ny + PH - 1) / PH)) return;              // block-uniform
    const int64_t py0 = (blk / ppr) * PH, px0 = (blk % ppr) * PW;
    int64_t cell[CELLS];
    bool live[CELLS];
#pragma unroll
    for (int q = 0; q < CELLS; ++q) {
        const int64_t yy = py0 + q * 8 + (t >> 5), xx = px0 + (t & 31);
        live[q] = yy < ny && xx < nx;
        cell[q] = yy * nx + xx;
    }
    double acc[CELLS];
#pragma unroll
    for (int q = 0; q < CELLS; ++q) acc[q] = 0.0;
    if (!skip_sums) {
        double px[CELLS], py[CELLS], pz[CELLS];
#pragma unroll
        for (int q = 0; q < CELLS; ++q) {
            px[q] = live[q] ? gxyz[cell[q]] : 0.0;
            py[q] = live[q] ? gxyz[n + cell[q]] : 0.0;
            pz[q] = live[q] ? gxyz[2 * n + cell[q]] : 0.0;
        }
        int64_t j0 = 0, j1 = m;
        const bool windowed = glat && olat;
        if (windowed) {                                         // latitude span of this block's cells -> observation index range
            double lo = 1e9, hi = -1e9;
#pragma unroll
            for (int q = 0; q < CELLS; ++q)
                if (live[q]) { const double la = glat[cell[q]]; lo = fmin(lo, la); hi = fmax(hi, la); }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o, kWave)); hi = fmax(hi, __shfl_xor(hi, o, kWave)); }
            if ((t & 63) == 0) { W.s_lo[t >> 6] = lo; W.s_hi[t >> 6] = hi; }
            __syncthreads();
            if (t == 0) {
                lo = fmin(fmin(W.s_lo[0], W.s_lo[1]), fmin(W.s_lo[2], W.s_lo[3]));
                hi = fmax(fmax(W.s_hi[0], W.s_hi[1]), fmax(W.s_hi[2], W.s_hi[3]));
                W.s_j[0] = lower_bound_lat(olat, m, lo - win_deg);
                W.s_j[1] = lower_bound_lat(olat, m, hi + win_deg + 1e-9);
            }
            __syncthreads();
            j0 = W.s_j[0];
            j1 = W.s_j[1];
        }
        const BlockSphere bs = block_sphere<CELLS>(px, py, pz, live, windowed ? cut_chord : 1e30, (double)INFINITY, W.red);
        f32x2 fx[CELLS], fy[CELLS], fz[CELLS];
#pragma unroll
        for (int q = 0; q < CELLS; ++q) {
            fx[q] = f32x2{(float)px[q], (float)px[q]};
            fy[q] = f32x2{(float)py[q], (float)py[q]};
            fz[q] = f32x2{(float)pz[q], (float)pz[q]};
        }
        const float fg2 = (float)g2;
        int fill = 0;
        for (int64_t c0 = j0; c0 < j1; c0 += 256) {
            {                                                   // one pass of 256 candidates: the survivors, in candidate order
                const int lane = t & 63, w = t >> 6;
                const int64_t c = c0 + t;
                double x = 0.0, y = 0.0, zz = 0.0;
                bool near = false;
                if (c < j1) {
                    x = oxyz[c]; y = oxyz[m + c]; zz = oxyz[2 * m + c];
                    const double dx = x - bs.cx, dy = y - bs.cy, dz = zz - bs.cz;
                    near = dx * dx + dy * dy + dz * dz <= bs.r2cull;
                }
                const unsigned long long mask = __ballot(near);
                if (lane == 0) W.wcnt[w] = __popcll(mask);
                __syncthreads();
                const int c0w = W.wcnt[0], c1w = W.wcnt[1], c2w = W.wcnt[2], c3w = W.wcnt[3];
                if (near) {
                    const int p = fill + (w > 0 ? c0w : 0) + (w > 1 ? c1w : 0) + (w > 2 ? c2w : 0) + __popcll(mask & ((1ull << lane) - 1ull));
                    lx[p] = (float)x; ly[p] = (float)y; lz[p] = (float)zz;
                    lw[p] = (float)(osig[c] * (z[c] - z0[c]));
                }
                fill += c0w + c1w + c2w + c3w;                  // <= kUpdStage: a pass starts at fill <= kUpdStage - 256
                if (t < 16 && fill + t < ((fill + 15) & ~15)) { // the padding behind the list (the next pass writes over it)
                    lx[fill + t] = 0.0f; ly[fill + t] = 0.0f; lz[fill + t] = 0.0f; lw[fill + t] = 0.0f;
                }
                __syncthreads();
            }
            if (fill + 256 > kUpdStage || c0 + 256 >= j1) {    // block-uniform
                for (int jb = 0; jb < fill; jb += 64) {         // 64 entries per fp32 partial sum (16 terms per lane), then double
                    const int je = jb + 64 < fill ? jb + 64 : fill;
                    f32x2 s0[CELLS], s1[CELLS];
#pragma unroll
                    for (int q = 0; q < CELLS; ++q) { s0[q] = f32x2{0.0f, 0.0f}; s1[q] = f32x2{0.0f, 0.0f}; }
#pragma unroll 2
                    for (int j = jb; j < je; j += 4) {          // wave-uniform addresses: broadcast reads
                        const f32x4 ox = *reinterpret_cast<const f32x4*>(lx + j), oy = *reinterpret_cast<const f32x4*>(ly + j);
                        const f32x4 oz = *reinterpret_cast<const f32x4*>(lz + j), ow = *reinterpret_cast<const f32x4*>(lw + j);
#pragma unroll
                        for (int q = 0; q < CELLS; ++q) {
                            s0[q] = far_pairs(fx[q] - ox.xy, fy[q] - oy.xy, fz[q] - oz.xy, fg2, ow.xy, s0[q]);
                            s1[q] = far_pairs(fx[q] - ox.zw, fy[q] - oy.zw, fz[q] - oz.zw, fg2, ow.zw, s1[q]);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < CELLS; ++q) {
                        acc[q] += (double)s0[q].x;
                        acc[q] += (double)s0[q].y;
                        acc[q] += (double)s1[q].x;
                        acc[q] += (double)s1[q].y;
                    }
                }
                fill = 0;
                __syncthreads();
            }
        }
    }
#pragma unroll
    for (int q = 0; q < CELLS; ++q) {
        if (live[q]) {
            const double v0 = inc0[cell[q]];
            const double v = skip_sums ? v0 : v0 + gsig[cell[q]] * acc[q];
            if (inc) inc[cell[q]] = (T)v;
            if (xa) xa[cell[q]] = (T)((double)xb[cell[q]] + v);
        }
    }
}
