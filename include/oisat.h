/*
 * oisat.h -- C-ABI of liboisat_hip.so: the MI355X (gfx950) implementation of the
 * optimal-interpolation hot path of ahsouri/OI-SAT-GMI.
 *
 * The reference has NO native/FFI layer: its boundary for this path is the Python call surface
 * (SURVEY.md section 8(b)).  This header is therefore the C-ABI *underneath* that surface -- what
 * the Python drop-in (oi-sat-gmi_amd/oisatgmi/) binds with ctypes, and what a maintainer of the
 * reference would bind from its own modules (stub shown in INTEGRATION.md).  Each entry point
 * names the reference code it replaces (file:line into the reference tree).
 *
 * Conventions
 *   - plain C: opaque handle, raw pointers, explicit int64 sizes; no torch / numpy types.
 *   - every function returns 0 on success, a negative OISAT_E* code on failure;
 *     oisat_last_error() gives the thread-local message.
 *   - "dev" pointers are HIP device pointers owned by the caller (e.g. torch tensors'
 *     data_ptr(), or memory from oisat_dmalloc).  Kernels are enqueued on the handle's stream
 *     (oisat_set_stream) and are asynchronous unless stated.  Internal workspaces are grow-only:
 *     a compute call allocates only when it meets a size larger than any before it on this handle
 *     (oisat_dense_reserve pre-sizes the dense path so that this never happens inside a timed or
 *     repeated region); nothing synchronises the device except where a host result is returned.
 *   - dtype: OISAT_F32 (0) or OISAT_F64 (1) selects the field element type; arithmetic is done
 *     in that type with the reference's operation order (no fast-math, no FMA contraction), and
 *     reductions always accumulate in double.
 */
#ifndef OISAT_H
#define OISAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OISAT_F32 0
#define OISAT_F64 1

#define OISAT_OK 0
#define OISAT_EINVAL (-1)   /* bad argument */
#define OISAT_EHIP (-2)     /* HIP runtime error */
#define OISAT_ENOMEM (-3)   /* device allocation failed */
#define OISAT_ENOTPD (-4)   /* Cholesky met a non-positive pivot */
#define OISAT_ENODEV (-5)   /* no usable gfx950 device */

#define OISAT_MAX_SCALES 128

typedef struct oisat_ctx oisat_ctx;

/* ---- lifetime, errors, memory, stream -------------------------------------------------------- */
int oisat_init(int device_id, oisat_ctx** out);
void oisat_shutdown(oisat_ctx* h);
const char* oisat_last_error(void);
const char* oisat_version(void);
int oisat_device_info(oisat_ctx* h, char* name_out, int name_cap, int* cu_count, int64_t* hbm_bytes);

int oisat_set_stream(oisat_ctx* h, void* hip_stream);       /* NULL = the default stream */
int oisat_stream_create(oisat_ctx* h);                      /* give this handle its own non-blocking stream: several
                                                               handles on one device then run concurrently (tiles) */
int oisat_stream_create_masked(oisat_ctx* h, int reserve_per_xcd); /* like oisat_stream_create, but the stream's kernels keep
                                                               off `reserve_per_xcd` CUs of every XCD (hipExtStreamCreateWithCUMask):
                                                               used for the bulk group of a BatchedFactor so that the dependent
                                                               chain of the critical group finds CUs free of GEMM waves.  Such a
                                                               stream synchronises with the NULL stream (HIP: it is a blocking one) */
int oisat_bind_thread(oisat_ctx* h);                        /* hipSetDevice(handle's device) for the CALLING host thread:
                                                               HIP's current device is per thread, so a worker thread that
                                                               drives a handle calls this once before anything else.  One
                                                               handle is driven by one host thread at a time. */
int oisat_wait_for(oisat_ctx* waiter, oisat_ctx* signaler); /* work enqueued on waiter's stream after this call starts only
                                                               when everything enqueued on signaler's stream so far is
                                                               done (event record + stream wait; nothing blocks the host) */
int oisat_sync(oisat_ctx* h);                               /* hipStreamSynchronize(stream) */
int oisat_query(oisat_ctx* h, int* busy);                   /* hipStreamQuery(stream): *busy = 1 while work is in flight;
                                                               lets a host that drives several handles serve whichever
                                                               finishes first (BatchedFactor: a group's solves are released
                                                               when THAT group is factored, whatever the enqueue order) */
int oisat_dmalloc(oisat_ctx* h, size_t bytes, void** dev_out);
int oisat_dfree(oisat_ctx* h, void* dev);
int oisat_h2d(oisat_ctx* h, void* dev_dst, const void* host_src, size_t bytes);   /* async on stream */
int oisat_d2h(oisat_ctx* h, void* host_dst, const void* dev_src, size_t bytes);   /* synchronises */
int oisat_memset(oisat_ctx* h, void* dev, int byte_value, size_t bytes);

/* per-kernel HIP-event timing (bench.py roofline leg).  Off by default. */
int oisat_prof_enable(oisat_ctx* h, int on);
int oisat_prof_reset(oisat_ctx* h);
/* synchronises; writes up to cap records; returns the number of distinct kernels (>=0) */
int oisat_prof_collect(oisat_ctx* h, int cap, char (*names)[64], double* total_ms, int64_t* launches);

/* ---- element-wise OI: optimal_interpolation.py:6-52 ------------------------------------------ */
/* Regularisation sweep, optimal_interpolation.py:26-33: for each scale s,
 *   t = Sa*s; K = t*(t+So)^-1; Sb = (1-K)*t; AK = 1 - Sb/t; mean_s = nanmean(AK).
 * Sa, So: dev, n elements.  scales: HOST doubles (1 <= nscales <= OISAT_MAX_SCALES, else OISAT_EINVAL).
 * mean_out / count_out: HOST arrays of nscales (sum of non-NaN AK / count; count of non-NaN; count_out may be NULL).
 * Synchronises (returns host values).  Deterministic: fixed launch shape, fixed reduction order.
 * The means are taken over AK = K (Sb/t = 1 - K in real arithmetic; NaN where t == 0, as 0/0 is), one division per cell and
 * scaling: each is within 1.5 * 2^-52 ABSOLUTE of the mean of the reference's 1 - Sb/t wherever 0 <= K <= 1.  That is nothing
 * on curves of 0.1 .. 1, and it is the reference form's own rounding noise: where Sa/So is near 1e-10 the means are
 * 1e-11 .. 1e-9, the reference's curve is this one plus that noise, and Kneedle finds a knee in the noise that the smooth
 * curve does not have (oisat_oi_fused then answers index 0 where the reference picks some index of its noise). */
int oisat_oi_curve(oisat_ctx* h, int dtype, const void* Sa, const void* So, int64_t n,
                   const double* scales, int nscales, double* mean_out, int64_t* count_out);

/* Analysis for ONE scale, optimal_interpolation.py:14 and :46-52:
 *   Y[Y<0] = 0 (written back in place), K, AK, Sb as above, inc = K*(Y-Xa), Xb = Xa+inc,
 *   err = sqrt(Sb).  All dev, n elements; any of Xb/AK/inc/err may be NULL to skip it. */
int oisat_oi_apply(oisat_ctx* h, int dtype, const void* Xa, void* Y_inout, const void* Sa,
                   const void* So, int64_t n, double scale, void* Xb, void* AK, void* inc, void* err);

/* Fully device-side OI: sweep + knee pick (Kneedle, the algorithm of kneed.KneeLocator used at
 * optimal_interpolation.py:37-41, restated) + analysis, no host round trip; graph-capturable.
 * index_dev: dev int32[1] receives the chosen index; curve_dev: dev double[nscales] (may be NULL).
 * forced_index >= 0 (< nscales) bypasses the pick; with fewer than three scales the index is 0.  When the library is to pick
 * (forced_index < 0, nscales >= 3) the LAST entry of scales must be finite and no smaller than any other entry, else
 * OISAT_EINVAL and nothing is written: the walk ends at the table's maximum, and past a maximum that is not the last point it
 * would look one element beyond the difference curve (kneed itself raises IndexError on such a table). */
int oisat_oi_fused(oisat_ctx* h, int dtype, const void* Xa, void* Y_inout, const void* Sa,
                   const void* So, int64_t n, const double* scales, int nscales, int forced_index,
                   void* Xb, void* AK, void* inc, void* err, int32_t* index_dev, double* curve_dev);

/* ---- monthly averaging: averaging.py:11-24 and :97-108 ---------------------------------------- */
/* out[c] = nanmean_k stack[k][c]  (np.nanmean(axis=0), sequential-k summation like numpy).
 * stack: dev, k*n contiguous.  inf_to_nan != 0 first maps +/-inf to NaN (averaging.py:92). */
int oisat_nanmean_stack(oisat_ctx* h, int dtype, const void* stack, int k, int64_t n, int inf_to_nan, void* out);

/* error_averager, averaging.py:11-24: per cell drop NaN/inf, out = sqrt(sum / count^2);
 * count 0 -> NaN.  square_input != 0: stack holds sigma and is squared first (averaging.py:101). */
int oisat_error_average(oisat_ctx* h, int dtype, const void* stack, int k, int64_t n, int square_input, void* out);

/* Device-resident month (oisatgmi/month.py): the two reductions above, granule by granule.  acc: dev block of
 * 5*n elements of acc_dtype (running sums) followed by 5*n uint32 (counts), zeroed before the first granule, for
 * the fields vcd (mean, inf -> NaN), uncertainty (error kind, squared), ctm_vcd, new_amf, old_amf (plain means).
 * One launch per granule folds its five n-element fields into acc in the order of the launches; bit f of
 * f32_mask says field f is float32 (else float64); it is converted to acc_dtype in registers.  kept: dev int32,
 * the launch does nothing when *kept == 0.  Summing granule by granule from 0 gives the bits of the stack kernels. */
int oisat_month_accumulate(oisat_ctx* h, int acc_dtype, const void* vcd, const void* uncertainty, const void* ctm_vcd,
                           const void* new_amf, const void* old_amf, int f32_mask, int64_t n, const int32_t* kept, void* acc);
/* out: dev [5][n] of acc_dtype, the finished means (and the error average for field 1) of acc. */
int oisat_month_finish(oisat_ctx* h, int acc_dtype, const void* acc, int64_t n, void* out);
/* *kept = 0 when every element of x is NaN, else 1 (interpolator.py's `np.isnan(vcd).all()` skip test). */
int oisat_all_nan(oisat_ctx* h, int dtype, const void* x, int64_t n, int32_t* kept);
/* out[i] = (double)x[i] (exact; NumPy's astype(float64) of a float32 array). */
int oisat_widen(oisat_ctx* h, const float* x, int64_t n, double* out);

/* out = (x - offset) / slope  (bias_correct, driver.py:65-106) or x / divisor with offset 0
 * (O3 unit conversion, driver.py:62-63). */
int oisat_affine(oisat_ctx* h, int dtype, const void* x, int64_t n, double offset, double slope, void* out);

/* Sa = (Xa*error_ctm/100)^2 and So = err^2, the argument wiring of oisatgmi.oi, driver.py:110-114 */
int oisat_oi_variances(oisat_ctx* h, int dtype, const void* Xa, const void* sat_err, int64_t n,
                       double error_ctm, void* Sa_out, void* So_out);

/* Emission scaling factor written to the output file: posterior/prior with NaN, +/-inf and 0 mapped to 1.0
 * (write_to_nc, driver.py:204-206). */
int oisat_scaling_factor(oisat_ctx* h, int dtype, const void* posterior, const void* prior, int64_t n, void* out);

/* ---- AMF recalculation (upstream of the averaging): amf_recal.py ---------------------------------------- */
/* Model partial column deltap*profile/g/Mair*N_A*1e-4*1e-15*100*1e-9, left to right in `dtype` (:51-56).
 * profile == NULL: the air column deltap/g/Mair*N_A*1e-4*1e-15*100 (ak_conv_mopitt.py:66). */
int oisat_partial_column(oisat_ctx* h, int dtype, const void* deltap, const void* profile, int64_t n, void* out);

/* Per-pixel vertical interpolation and AMF (the Python double loop :93-119 plus the record update :176-182):
 * scattering weights interpolated in log-pressure onto the model levels (scipy interp1d, linear,
 * fill_value="extrapolate": stable sort, searchsorted-left, clipped end segments), inf -> 0, tropopause
 * mask, model SCD / VCD by nansum in NumPy's pairwise order, new AMF = SCD/VCD (NaN if VCD == 0),
 * vcd_out = amf*vcd/new_amf, ctm_vcd = model VCD (NaN where vcd_out is NaN/inf).
 * Cubes are level-major [nz][n]; satellite cubes double, model cubes of ctm_dtype (np.log and the VCD
 * nansum are evaluated in that dtype, as NumPy does); nzs <= 64, nzc <= 128; tropopause may be NULL. */
int oisat_amf_recal(oisat_ctx* h, const double* sat_pmid, const double* sat_sw, int nzs, int ctm_dtype,
                    const void* ctm_pmid, const void* ctm_partial, int nzc, const double* tropopause, const double* vcd,
                    const double* amf, int64_t n, double* new_amf, double* vcd_out, double* ctm_vcd);

/* No scattering weights (:160-171): ctm_vcd = nansum over levels of the partial columns (levels with
 * p < tropopause dropped when tropopause != NULL), NaN where vcd is NaN; cube and output in `dtype`. */
int oisat_column_sum(oisat_ctx* h, int dtype, const void* ctm_pmid, const void* ctm_partial, int nzc,
                     const double* tropopause, const double* vcd, int64_t n, void* ctm_vcd);

/* ---- averaging-kernel convolution: ak_conv_mopitt.py / ak_conv_gosat.py (driver.py:46-51 conv_ak) ------------
 * The satellite_opt counterpart of oisat_amf_recal: per pixel the model column (cubes of dtype ctm_dtype,
 * level-major [nzc][n]) is interpolated in log-pressure onto the satellite levels (double, [nzs][n]) with
 * scipy interp1d's arithmetic, then the retrieval's averaging kernels are applied.  np.log / np.log10 of a float32
 * cube is the double logarithm rounded once to float32.
 * Which arithmetic interp1d uses depends on the dtype and the fill value, and so does this library:
 *   - float32 cubes (either sensor) and GOSAT's fill_value="extrapolate": interp1d._call_linear -- stable sort with NaN
 *     last, searchsorted-left, end segments clipped, slope*(x - x_lo) + y_lo with the slope in the cubes' dtype;
 *   - float64 cubes under MOPITT's fill_value=nan: interp1d._call_linear_np, i.e. np.interp -- the node's own value
 *     when a level lies exactly on a node (of equal nodes, the last one's), and where the left-hand expression is NaN
 *     the same slope taken from the right-hand node, then the common value if both nodes hold it.
 * MOPITT (ak_conv_mopitt.py:118-146): fill NaN outside the model's pressure range; averaging_kernels is
 *   [nzs+1][n] (row 0 = surface); model_vcd = aprior_column + nansum(AK[1:]*(log10 x - log10 apriori_profile))
 *   + AK[0]*(log10 x_model[0] - log10 apriori_surface); model_xcol = 1e6*model_vcd/nansum(air partial column);
 *   pixels with NaN vcd are skipped (both NaN), +/-inf vcd -> model_vcd NaN.
 * GOSAT (ak_conv_gosat.py:118-143): linear extrapolation; model_xcol = nansum over levels of
 *   pressure_weight*(apriori + AK*(x - apriori)) with non-positive terms dropped; NaN/inf x_col -> NaN. */
int oisat_ak_conv_mopitt(oisat_ctx* h, int ctm_dtype, const void* ctm_pmid, const void* ctm_profile,
                         const void* ctm_air_partial, int nzc, const double* sat_pmid,
                         const double* averaging_kernels, const double* apriori_profile, int nzs,
                         const double* aprior_column, const double* apriori_surface, const double* vcd,
                         int64_t n, double* model_vcd, double* model_xcol);
int oisat_ak_conv_gosat(oisat_ctx* h, int ctm_dtype, const void* ctm_pmid, const void* ctm_profile, int nzc,
                        const double* sat_pmid, const double* averaging_kernels,
                        const double* apriori_profile, const double* pressure_weight, int nzs,
                        const double* x_col, int64_t n, double* model_xcol);

/* ---- model precipitable water for SSMIS: pwv_cal.py (driver.py:42-44 cal_pwv) ---------------------------------
 * oisat_water_column: deltap*profile/g/10000 per level, left to right in `dtype` (:63,:70).
 * oisat_pwv_sum: out = nansum_k(partial[k]/1000) level after level in `dtype`, NaN where the observation
 * (double vcd[n]) is NaN or +/-inf (:96-98).  partial: dev [nz][n] (after the optional model upscaling). */
int oisat_water_column(oisat_ctx* h, int dtype, const void* deltap, const void* profile, int64_t n, void* out);
int oisat_pwv_sum(oisat_ctx* h, int dtype, const void* partial, int nz, const double* vcd, int64_t n, void* out);

/* ---- regridding: interpolator.py:10-97 --------------------------------------------------------- */
/* signal.convolve2d(Z, ones(ky,kx)/(kx*ky)^(1|2), boundary='symm', mode='same'),
 * interpolator.py:40-46,:72-76.  Z, out: dev Ny*Nx row-major.  variance != 0 -> /(kx*ky)^2. */
int oisat_boxfilter_symm(oisat_ctx* h, int dtype, const void* Z, int64_t Ny, int64_t Nx, int ky, int kx,
                         int variance, void* out);

/* Bounded-radius exact nearest neighbour (what cKDTree.query + the `dists > 2*threshold` mask
 * need, interpolator.py:145-150,:78-91,:28-33).  Points/targets: dev double lon/lat arrays.
 * idx_out: dev int32[T], -1 where no point lies within max_dist (those cells are NaN-masked by
 * the caller's gather).  Exact ties resolve to the lowest point index (see oisat_nn_query_ties).  Distances are Euclidean in
 * degree space in double, like the reference: d2 = dx*dx + dy*dy without contraction, dist = sqrt(d2), and a target is kept
 * iff NOT dist > max_dist (a point at exactly max_dist is kept).  The answer is the brute-force one for every target: the
 * hash cell is the radius padded by 2^-26, which covers the rounding of the cell coordinates (csrc/regrid.hip).
 * NaN coordinates: a point with a NaN longitude or latitude is never returned and never counts as a tie; a target with a
 * NaN coordinate gets idx -1 and dist +inf; with no finite point at all every target does.  Coordinates must not be
 * infinite.  dist_out: +inf where idx is -1.  Synchronises internally (sizes a workspace). */
int oisat_nn_query(oisat_ctx* h, const double* plon, const double* plat, int64_t P,
                   const double* tlon, const double* tlat, int64_t T, double max_dist,
                   int32_t* idx_out, double* dist_out /* may be NULL */);

/* Same search, and additionally reports the targets whose nearest point is NOT unique: tie_list (dev int32[T])
 * receives, in no particular order, the ids of the kept targets for which a second point lies at the same distance
 * (to within 8 ulp of the squared distance); *n_ties (host) = how many.  Where the minimum is unique it is what
 * cKDTree(points).query(xi) returns (interpolator.py:82-88); where it is not, the reference's answer is whichever
 * of the equidistant nodes scipy's tree traversal meets first, so the host side re-queries exactly the listed
 * targets against that tree and patches idx_out (oisatgmi/interpolator.py: NNIndex.query_device).  This happens on
 * the reference's own MOPITT / GOSAT settings: grid_size 1.0 (reader.py:1209,:1271) against a model longitude
 * spacing of 1.25 or 2.5 degrees puts every other model centre midway between two fine-grid nodes. */
int oisat_nn_query_ties(oisat_ctx* h, const double* plon, const double* plat, int64_t P,
                        const double* tlon, const double* tlat, int64_t T, double max_dist,
                        int32_t* idx_out, double* dist_out /* may be NULL */,
                        int32_t* tie_list, int64_t* n_ties);

/* out[f][t] = idx[t] >= 0 ? values[f][idx[t]] : NaN  for nfields stacked fields
 * (the `Z.ravel()[idx]` + mask of _interpolosis type 2/4, interpolator.py:17-20,:28-33). */
int oisat_gather_mask(oisat_ctx* h, int dtype, const void* values, int64_t P, int nfields,
                      const int32_t* idx, int64_t T, void* out);

/* LinearNDInterpolator(tri, values, fill_value=nan) evaluated at T targets for nfields stacked fields
 * (_interpolosis type 1, interpolator.py:12-16).  The Delaunay triangulation is built by qhull on the
 * host as in the reference (:153) and handed over as its arrays: simplices int32[ns][3], neighbors
 * int32[ns][3] (-1 = hull), transform double[ns][3][2] (scipy layout: Tinv rows, then the offset
 * vertex), vertex_to_simplex int32[P].  nn_idx: nearest swath pixel per target from oisat_nn_query
 * (-1: masked -> NaN); the point-location walk starts there.  Outside the hull -> NaN.  When the walk meets a
 * degenerate simplex or does not converge it falls back, like scipy's _find_simplex_directed, to the brute-force scan
 * (_find_simplex_bruteforce: bounding box, every simplex, eps_broad towards NaN-transform simplices).
 * bounds_host: HOST double[4] = {min x, max x, min y, max y} of the triangulated points (Delaunay.min_bound /
 * max_bound) for that scan's bounding-box test; NULL = no box test.
 * The walk takes the first hull facet it crosses (a coordinate below -eps whose neighbour is -1) as "outside", without a
 * second look, as scipy's directed walk does.  Where the triangulation is not a partition to rounding -- qhull closes the
 * straight edge of a regular swath grid with zero-area slivers, and a target ON that edge is inside or outside by 1e-13 --
 * the answer therefore depends on the simplex the walk starts from: here always one at the target's nearest point
 * (vertex_to_simplex[nn_idx]; simplex 0 if that entry is out of range), in scipy the simplex its previous target ended in,
 * so for such hull-grazing targets scipy's own answer varies with the order of the targets and the two can differ.  They are
 * not reported by oisat_linear_locate unless a second simplex accepts them. */
int oisat_linear_interp(oisat_ctx* h, int dtype, const double* tlon, const double* tlat, int64_t T,
                        const int32_t* nn_idx, const int32_t* vertex_to_simplex, const int32_t* simplices,
                        const int32_t* neighbors, const double* transform, int64_t nsimplex,
                        const void* values, int64_t P, int nfields, void* out, const double* bounds_host);

/* scipy's Delaunay.transform on the device (the host computes it with three LAPACK calls per simplex: 0.55-1.0 s for the
 * 197,000 simplices of an OMI granule, more than qhull).  points: dev double[P][2] as Delaunay.points; simplices: dev
 * int32[nsimplex][3]; transform_out: dev double[nsimplex][3][2] = (T^-1 rows, r_2), NaN for a simplex whose 2 x 2 matrix
 * is singular or has a 1-norm condition number above 1 / (1000 eps), as scipy marks it.  Same elimination order as LAPACK's
 * (the values agree with scipy's to the last bit on the build host).  suspects (dev int32[nsimplex]) receives, in no
 * particular order, the simplices within four orders of magnitude of that limit or singular, *n_suspect (host) how many:
 * scipy's own decision and values for exactly those are a call of its routine on that subset (interpolator.py host side). */
int oisat_tri_transform(oisat_ctx* h, const double* points, int64_t P, const int32_t* simplices, int64_t nsimplex,
                        double* transform_out, int32_t* suspects, int64_t* n_suspect);

/* Targets whose location in the triangulation is NOT unique: amb_list (dev int32[T], no particular order) receives the
 * ids of the targets for which a second simplex accepts the point as well (it lies on a shared facet or vertex to within
 * scipy's eps) or whose walk had to fall back to the brute-force scan; *n_amb (host) = how many.  scipy evaluates targets
 * sequentially and starts every walk where the previous one ended (LinearNDInterpolator -> qhull._find_simplex with a
 * carried `start`), so for such targets the simplex -- and, next to a NaN vertex, the NaN pattern of interpolator.py:12-16 --
 * depends on the order of evaluation.  The normal case for level-3 lattice products (MOPITT, reader.py:1150-1211: every
 * fine node on the diagonal of a lattice square).  The host locates the listed targets with the same sequential search
 * (Delaunay.find_simplex over the whole target list) and passes the result to oisat_linear_interp_forced. */
int oisat_linear_locate(oisat_ctx* h, const double* tlon, const double* tlat, int64_t T, const int32_t* nn_idx,
                        const int32_t* vertex_to_simplex, const int32_t* simplices, const int32_t* neighbors,
                        const double* transform, int64_t nsimplex, int64_t P, const double* bounds_host,
                        int32_t* amb_list, int64_t* n_amb);

/* oisat_linear_interp with per-target simplices from the host: forced dev int32[T]; -2 = locate on the device (walk),
 * -1 = outside the triangulation (NaN), >= 0 = evaluate in that simplex. */
int oisat_linear_interp_forced(oisat_ctx* h, int dtype, const double* tlon, const double* tlat, int64_t T,
                               const int32_t* nn_idx, const int32_t* vertex_to_simplex, const int32_t* simplices,
                               const int32_t* neighbors, const double* transform, int64_t nsimplex,
                               const void* values, int64_t P, int nfields, void* out, const double* bounds_host,
                               const int32_t* forced);

/* RBFInterpolator(points, values, neighbors=5)(targets) for nfields stacked fields (_interpolosis type 3,
 * interpolator.py:21-27): thin-plate-spline kernel, degree-1 polynomial tail, no smoothing; per target the
 * `neighbors` (3..5, = min(5, P) in scipy) nearest points, ids sorted ascending, one (neighbors+3)^2 system
 * solved in double.  nn_idx: nearest point per target from oisat_nn_query with max_dist = cell (the mask
 * radius 2*threshold); targets with nn_idx < 0 are NaN after the reference's mask and get no value here
 * (oisat_rbf_check_masked looks at their neighbourhoods).  A NaN value makes every target whose
 * neighbourhood holds it NaN (as dgesv does).  *n_singular (host, may be NULL) = number of evaluated
 * targets whose system had a zero pivot (scipy raises LinAlgError("Singular matrix")); those targets are
 * written NaN.  Synchronises internally. */
int oisat_rbf_interp(oisat_ctx* h, int dtype, const double* plon, const double* plat, int64_t P,
                     const double* tlon, const double* tlat, int64_t T, const int32_t* nn_idx, double cell,
                     int neighbors, const void* values, int nfields, void* out, int64_t* n_singular);

/* oisat_rbf_interp that also reports the targets whose K-th neighbour is not unique (the runner-up is exactly as near):
 * which of the candidates RBFInterpolator's own KDTree(y).query(x, K) returns is a property of scipy's tree, and a regular
 * lattice of points (an L3 product) produces such targets wholesale.  tie_list: dev int32[T], *n_ties (host) entries filled,
 * in no particular order; their values in `out` come from the lowest-index choice and their zero pivots are NOT in
 * *n_singular -- send them through oisat_rbf_interp_forced with the neighbours the host's tree names. */
int oisat_rbf_interp_ties(oisat_ctx* h, int dtype, const double* plon, const double* plat, int64_t P,
                          const double* tlon, const double* tlat, int64_t T, const int32_t* nn_idx, double cell,
                          int neighbors, const void* values, int nfields, void* out, int64_t* n_singular,
                          int32_t* tie_list, int64_t* n_ties);

/* Type-3 evaluation of n listed targets on neighbourhoods given by the caller: targets dev int32[n] (indices into the T
 * targets), ids dev int32[n * neighbors] (point indices, any order; an entry outside [0, P) leaves that target as it is).
 * Overwrites out[f * T + target] for every field; *n_singular (host, may be NULL) = zero pivots among them. */
int oisat_rbf_interp_forced(oisat_ctx* h, int dtype, const double* plon, const double* plat, int64_t P,
                            const double* tlon, const double* tlat, int64_t T, const int32_t* targets,
                            const int32_t* ids, int64_t n, int neighbors, const void* values, int nfields, void* out,
                            int64_t* n_singular);

/* The other half of interpolator.py:21-27: scipy evaluates RBFInterpolator at EVERY target and masks afterwards,
 * so a singular neighbourhood raises LinAlgError for the whole call even when its target is masked (a regular
 * lattice of points and a target beyond its edge: five collinear neighbours).  For the targets with nn_idx < 0:
 * the `neighbors` nearest points are found (two-level search on a hash of at most 128 x 128 cells, so that a
 * target a whole domain away from every point costs no more than a near one), the system is factored, and
 * *n_singular (host) = number of zero pivots met.  Independent of the values: once per (points, targets) pair.
 * Synchronises internally. */
int oisat_rbf_check_masked(oisat_ctx* h, const double* plon, const double* plat, int64_t P, const double* tlon,
                           const double* tlat, int64_t T, const int32_t* nn_idx, double cell, int neighbors,
                           int64_t* n_singular);

/* _upscaler fused (interpolator.py:72-91): box-average of the ky*kx window around fine node
 * idx[t] (symmetric boundary, NaN-poisoning, optional variance kernel), evaluated only at the
 * fine nodes the model cells pick; idx < 0 -> NaN.  Z: dev nfields*Ny*Nx; out: dev nfields*T. */
int oisat_boxfilter_pick(oisat_ctx* h, int dtype, const void* Z, int64_t Ny, int64_t Nx, int nfields,
                         int ky, int kx, int variance, const int32_t* idx, int64_t T, void* out);

/* out = mask_dev ? x*1 : NaN  -- the `field*mask` of interpolator.py:126-128,:163; square != 0
 * squares first (uncertainty**2*mask, :186).  flag: dev array of dtype, kept if flag > thresh. */
int oisat_flag_mask(oisat_ctx* h, int dtype, const void* x, const void* flag, int64_t n, double thresh,
                    int square, void* out);

int oisat_sqrt(oisat_ctx* h, int dtype, const void* x, int64_t n, void* out);      /* interpolator.py:188 */

/* ---- dense Gaussian-B analysis (north-star extension; no reference counterpart) ---------------- */
/* x_a = x_b + B H^T (H B H^T + R)^-1 (y - H x_b),  B = D^1/2 C D^1/2,
 * C_ij = exp(-|p_i - p_j|^2 * g),  g = R_earth^2/(2 L^2), p = unit vectors (chord distance).
 * Reduces to optimal_interpolation.py:27,:49-50 when L -> 0 and H selects grid cells.
 * All coordinates are double SoA [3][count]; S is float, row-major, leading dimension ld. */

/* S = sig_a sig_b C(a,b) + delta_ab var_a, written for the lower triangle by 64x64 tiles (diagonal
 * tiles complete) over mp = roundup(m,128) rows; rows/cols m..mp are identity padding.
 * S must hold mp rows of ld >= mp floats.  oxyz: dev double[3*m]. */
int oisat_cov_build(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m,
                    double g, float* S, int64_t ld);

/* d = y - xb[cell]  (innovation; dev double out). */
int oisat_innovation(oisat_ctx* h, int dtype, const void* xb, const int64_t* cell, const double* y,
                     int64_t m, double* d_out);

/* The one O(m^3) kernel of the factorization, exposed for tests and microbenchmarks:
 * mode 0: C -= A B^T, mode 1: C = A B^T.  C: M x N (ldc), A: M x K (lda), B: N x K (ldb), row-major,
 * K-contiguous operands; M, N multiples of 128, K of 32; lower != 0: C is anchored on the diagonal and only its
 * lower triangle is defined afterwards -- tiles strictly above the diagonal are skipped, at 128- or 64-row/column
 * granularity depending on the launch size, so entries above the diagonal may or may not have been updated.
 * fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32. */
int oisat_gemm_nt(oisat_ctx* h, float* C, int64_t ldc, const float* A, int64_t lda, const float* B, int64_t ldb,
                  int64_t M, int64_t N, int64_t K, int mode, int lower);

/* In-place blocked Cholesky S = L L^T: L in the lower triangle; the strictly-upper part is NOT part of the result
 * (inside the 128x128 diagonal tiles the trailing updates write it; elsewhere it is left untouched), fp32 MFMA
 * trailing updates.  info_host: 0 ok, j>0 = first non-positive pivot column (1-based). */
int oisat_potrf(oisat_ctx* h, float* S, int64_t m, int64_t ld, int* info_host);

/* ---- the covariance's latitude envelope ---------------------------------------------------------------------
 * With the observations in ASCENDING latitude order S is a band: a pair whose latitudes differ by more than the
 * angle of the library's cut-off chord (correlation below 2^-52, the cut-off of oisat_cov_residual and
 * oisat_apply_increment) contributes nothing, and a Cholesky factor has no fill outside the envelope of its matrix.
 *
 * oisat_envelope (host only, no device call): lat_sorted = host double[m], ascending, degrees.  Writes
 * env_out[0 .. nb) = first[i], the first 128-row tile column of tile row i that can hold a pair inside the cut-off
 * (tile k is outside when lat_max(tile k) < lat_min(tile i) - angle; non-decreasing; first[i] <= max(i - 1, 0)), and
 * env_out[nb .. 2 nb) = last[b] = max{ j : first[j] <= b };  nb = roundup(m, 128) / 128.  The caller keeps this
 * table on the host and a copy of all 2 nb words on the device.
 *
 * oisat_cov_build_env: oisat_cov_build for such a system.  env_dev = the DEVICE copy.  Tiles inside the envelope are
 * evaluated, the lower tiles outside it are FILLED WITH EXACT ZEROS (never left as they were).
 *
 * oisat_potrf_env: oisat_potrf of a matrix built by oisat_cov_build_env with the same table.  first = the HOST
 * table (checked: range, order), env_dev = its device copy (must stay valid and unchanged while the factor is in
 * use).  The task graph has tile tasks inside the envelope only and starts every K-loop at the envelope; inside the
 * envelope the factor has the bits of oisat_potrf's task-graph factor of the same zero-filled matrix, outside it
 * the zeros stay.  Systems the task graph does not take (under three block rows, OISAT_DAG=0) are factored densely.
 * The handle remembers the envelope with the factor: oisat_gain_solve and oisat_potrs sweep inside it (same bits: the
 * skipped blocks are zeros).  Who reads an enveloped factor, per function:
 *   oisat_gain_solve, oisat_potrs, oisat_trsm_rows_bwd     walk the envelope only
 *   oisat_trsm_rows, oisat_posterior_error, oisat_gain_diag, a download of S
 *                                                          read densely and find the zeros of the build
 *   oisat_potrf, oisat_factor_adopt                        forget the envelope (dense sweeps from then on)
 * OISAT_ENVELOPE=0 in the environment (read at every call) makes both entry points behave exactly as oisat_cov_build /
 * oisat_potrf: the dense path, for A/B timing and tests.
 *
 * oisat_factor_envelope (host only): the same table for the fp32 FACTOR, which oisat_gain_solve uses as a
 * preconditioner only (it refines against the float64 residual of the full S, cut off at 2^-52 as before).  Where the
 * factorization is bound by tile work (more than ~1 500 K-loop steps per block row inside the narrow table) the
 * table is cut at the factor's own, larger correlation (kFactorCutBits, csrc/dense_tables.hip); for every smaller
 * system, whose factorization is its chain, it is oisat_envelope's table word for word.  first[] is nowhere smaller
 * than oisat_envelope's.  This is the table DenseAnalysis.run() builds, factors and sweeps with.
 * OISAT_FACTOR_CUT_BITS=<n> in the environment (read at every call; 1 <= n <= 52, anything else is OISAT_EINVAL) forces
 * the cut-off 2^-n for every size; 52 reproduces oisat_envelope's table exactly. */
int oisat_envelope(const double* lat_sorted, int64_t m, double g, int32_t* env_out);
int oisat_factor_envelope(const double* lat_sorted, int64_t m, double g, int32_t* env_out);
/* The far stretch of the factor's K-loops (csrc/dense_tables.hip: kFactorFarBits).
 * oisat_factor_far (host only): far_out[i], first[i] <= far_out[i] <= i, = the first block column of block row i that is NOT
 * far: every correlation between an observation of block row i and one of a block column k < far_out[i] is below the far
 * cut-off.  The enveloped task graph runs the K-blocks first[i] <= k < far_out[i] of the row's tiles with both operands
 * rounded to bf16 (fp32 accumulation): the factor is oisat_gain_solve's preconditioner only.  first = the table of
 * oisat_factor_envelope (or oisat_envelope) for the same observations and g.  The stretch is on where
 * oisat_factor_envelope's rule picks the narrow table (tile-work-bound systems, no forced cut-off); everywhere else, and
 * under OISAT_ENVELOPE=0, far_out == first: no stretch, the factor's bits are those of the fp32 task graph.
 * OISAT_FACTOR_FAR_BITS=<n> in the environment (read at every call; 0 <= n <= 52, anything else is OISAT_EINVAL): 0 switches
 * the stretch off, n >= 1 forces the cut-off 2^-n at every enveloped size, also under a forced OISAT_FACTOR_CUT_BITS (an
 * n at or above the table's own cut-off leaves nothing far).
 * oisat_set_factor_far: hands the table (host int32[nb], copied; NULL / 0 = none) to the NEXT oisat_potrf_env /
 * oisat_potrf_env_fwd on this handle, which consumes it whatever its outcome and checks it against its own first.  Without
 * it, and in every other factorization (oisat_potrf, the batched ones), there is no far stretch. */
int oisat_factor_far(const double* lat_sorted, int64_t m, double g, const int32_t* first, int32_t* far_out);
/* The middle stretch of the factor's K-loops (csrc/dense_tables.hip: kFactorMidBits).
 * oisat_factor_mid (host only): mid_out[i], far[i] <= mid_out[i] <= i, = the first block column of block row i that is NOT
 * middle: every correlation between an observation of block row i and one of a block column k < mid_out[i] is below the
 * middle cut-off.  The enveloped task graph runs the K-blocks far[i] <= k < mid_out[i] of the row's tiles as split bf16
 * products: each operand a = hi + lo, hi = bf16(a), lo = bf16(a - hi), and a b^T becomes lo hi^T + hi lo^T + hi hi^T with fp32
 * accumulation (relative error ~2^-16 where the far stretch has 2^-8).  first and far are the tables of
 * oisat_factor_envelope and oisat_factor_far for the same observations and g (far == first: no far stretch, the middle one
 * starts at first[i]); the same argument checks as oisat_factor_far, and far is checked against first.  The stretch is on
 * exactly where the far stretch is on by default; everywhere else, and under OISAT_ENVELOPE=0, mid_out == far.
 * OISAT_FACTOR_MID_BITS=<n> in the environment (read at every call; 0 <= n <= 52, anything else is OISAT_EINVAL): 0 switches
 * the stretch off, n >= 1 forces the cut-off 2^-n at every enveloped size, whatever OISAT_FACTOR_FAR_BITS says (an n at or above
 * the far cut-off in force leaves nothing in the middle).
 * oisat_set_factor_mid: hands the table (host int32[nb], copied; NULL / 0 = none) to the NEXT oisat_potrf_env /
 * oisat_potrf_env_fwd on this handle, which consumes it whatever its outcome and checks it against its own first and the far
 * table set for the same call.  Without it, and in every other factorization, there is no middle stretch.  The ticket words
 * of oisat_dag_task_order_env do not carry it: the launch reads the table itself. */
int oisat_factor_mid(const double* lat_sorted, int64_t m, double g, const int32_t* first, const int32_t* far, int32_t* mid_out);
/* The near stretch of the factor's K-loops (csrc/dense_tables.hip: kFactorNearBits).
 * oisat_factor_near (host only): near_out[i], mid[i] <= near_out[i] <= i, = the first block column of block row i that is NOT
 * near.  The enveloped task graph runs the K-blocks mid[i] <= k < near_out[i] of the row's tiles as three-way split bf16
 * products: each operand a = hi + mid + lo, hi = bf16(a), mid = bf16(a - hi), lo = bf16(a - hi - mid) (nearest even; both
 * differences are exact), and a b^T becomes the eight products of those parts without lo lo^T, smallest first, with fp32
 * accumulation: the split is exact and what is dropped is at most 2^-32 of a term.  first and mid are the tables of oisat_factor_envelope and oisat_factor_mid (mid == far == first: the near
 * stretch starts at first[i]); the same argument checks as oisat_factor_mid, and mid is checked against first.  The stretch is
 * on exactly where the far and middle stretches are on by default; everywhere else, and under OISAT_ENVELOPE=0,
 * near_out == mid.
 * OISAT_FACTOR_NEAR_BITS in the environment (read at every call): 0 switches the stretch off (near_out == mid: the launch
 * without the stretch, bit for bit); 1 <= n <= 52 forces the table of cut-off 2^-n at every enveloped size; `all` forces the
 * whole rest of every row, near_out[i] = i; anything else is OISAT_EINVAL.
 * oisat_set_factor_near: hands the table (host int32[nb], copied; NULL / 0 = none) to the NEXT oisat_potrf_env /
 * oisat_potrf_env_fwd on this handle, which consumes it whatever its outcome and checks it against its own first and the far
 * and middle tables set for the same call.  Without it, and in every other factorization, there is no near stretch.  The
 * ticket words do not carry it, and the launch that also solves (oisat_batch_analyse) ignores it. */
int oisat_factor_near(const double* lat_sorted, int64_t m, double g, const int32_t* first, const int32_t* mid, int32_t* near_out);

/* ---- the correlation model ----------------------------------------------------------------------------------------
 * OISAT_CORR_GAUSSIAN (default): C = exp(-g chord^2).  OISAT_CORR_GASPARI_COHN: the compactly supported fifth-order function
 * of Gaspari and Cohn (1999, eq. 4.10) matched to the same g (half-support c = L sqrt(10/3): z = chord sqrt(0.6 g)),
 *   0 <= z <= 1:  C = -z^5/4 + z^4/2 + 5 z^3/8 - 5 z^2/3 + 1
 *   1 <  z <  2:  C = z^5/12 - z^4/2 + 5 z^3/8 + 5 z^2/3 - 5 z + 4 - 2/(3 z)
 *   z >= 2:       C = 0 exactly
 * It takes no parameter besides g.  Its latitude windows, envelopes and culls end at the support chord 2 / sqrt(0.6 g) and
 * leave out exact zeros only.
 * OISAT_CORR_SOAR: the second-order autoregressive function of classical optimal interpolation, the Matern function of
 * nu = 3/2 matched to the same g,
 *   C = (1 + s) exp(-s),  s = chord sqrt(2 g) = distance / L      (C ~ 1 - g chord^2 at small separation, C(0) = 1 exactly)
 * Once mean-square differentiable, exponential tails: it reaches 2^-52 at s = 39.75 (the Gaussian: 8.49 L), so from L ~ 321 km
 * on nothing is windowed.  Positive definite in R^3, hence on the sphere with chord distance.  No parameter besides g, no
 * far tier (oisat_solve_tier_counts: far_out = 0).  Its code is 3 = 2 nu; 2 is no model and stays OISAT_EINVAL.
 * oisat_set_correlation: the model of every later oisat_cov_build*, oisat_cov_residual, oisat_gain_solve,
 * oisat_apply_increment*, oisat_posterior_error and oisat_batch_solve on this handle (set it per run where handles are
 * shared, like oisat_set_refine_tol).  oisat_batch_analyse is Gaussian only: OISAT_EINVAL under any other model.
 * oisat_corr_eval (host only): out[i] = C at squared chord d2[i], float64, by the function the float64 kernels use.
 * oisat_corr_cut_chord (host only): the chord at which C has fallen to 2^-bits (bits >= 1) -- Gaussian sqrt(bits / (g log2 e));
 * Gaspari-Cohn by bisection, never beyond the support chord, and the support chord itself from 52 bits on; SOAR by bisection
 * on s (15.265708 at 18 bits, 22.568011 at 28, 39.751137 at 52), not clamped to the sphere's diameter 2.
 * oisat_envelope_corr / oisat_factor_envelope_corr / oisat_factor_far_corr: the three tables above for a model; kind =
 * OISAT_CORR_GAUSSIAN gives the tables of the functions above word for word.  Under any other model the factor's envelope is
 * the 2^-52 envelope (= oisat_envelope_corr; Gaspari-Cohn: the support envelope) and far_out == first unless
 * OISAT_FACTOR_CUT_BITS / OISAT_FACTOR_FAR_BITS force a cut-off: the Gaussian's defaults were measured for the Gaussian.  An
 * unknown kind is OISAT_EINVAL. */
#define OISAT_CORR_GAUSSIAN 0
#define OISAT_CORR_GASPARI_COHN 1
#define OISAT_CORR_SOAR 3                  /* = 2 nu of the Matern family; 2 is unassigned and stays OISAT_EINVAL */
int oisat_set_correlation(oisat_ctx* h, int kind);
int oisat_corr_eval(int kind, double g, const double* d2, int64_t n, double* out);
int oisat_corr_cut_chord(int kind, double g, double bits, double* chord_out);
/* The far tier of the float64 sums (Gaussian only; csrc/dense_solve_dev.inc: kSolveFarBits): the increment
 * and the compact-block residual evaluate an observation whose correlation with every point of a workgroup's block is below
 * 2^-bits in fp32 and add the block's fp32 partial sum to the float64 one.  By default the increment does so at 2^-28 and the residual
 * does not.  OISAT_SOLVE_FAR_BITS=<b> in the environment (read at every call): 0 = no tier (every pair in float64, the fields
 * of the code before the tier, byte for byte), 0 < b <= 52 = the tier at 2^-b in both (at 52 the far radius is the cull's: the list stays empty); anything else is OISAT_EINVAL
 * of the call.
 * oisat_solve_tier_counts (host only): for ONE block of points pts_xyz = x[npts] | y[npts] | z[npts] (unit vectors) and the
 * observations obs_xyz = x[m] | y[m] | z[m], the number of observations the block evaluates in float64 (near_out) and in fp32
 * (far_out); the rest is culled.  olat = the observations' latitudes, ascending, with [lat_lo, lat_hi] the latitude span of the
 * block's points (the kernels' window), or NULL: no window, no cull, nothing far.  bits as in the variable; < 0 = the library's
 * current setting.  Either out pointer may be NULL. */
int oisat_solve_tier_counts(int kind, double g, double bits, const double* pts_xyz, int64_t npts, const double* obs_xyz, int64_t m,
                            const double* olat, double lat_lo, double lat_hi, int64_t* near_out, int64_t* far_out);
int oisat_envelope_corr(int kind, const double* lat_sorted, int64_t m, double g, int32_t* env_out);
int oisat_factor_envelope_corr(int kind, const double* lat_sorted, int64_t m, double g, int32_t* env_out);
int oisat_factor_far_corr(int kind, const double* lat_sorted, int64_t m, double g, const int32_t* first, int32_t* far_out);
int oisat_set_factor_far(oisat_ctx* h, const int32_t* far, int64_t nb);
int oisat_factor_mid_corr(int kind, const double* lat_sorted, int64_t m, double g, const int32_t* first, const int32_t* far,
                          int32_t* mid_out);       /* oisat_factor_mid for a model; not Gaussian: mid_out == far unless forced */
int oisat_set_factor_mid(oisat_ctx* h, const int32_t* mid, int64_t nb);
int oisat_factor_near_corr(int kind, const double* lat_sorted, int64_t m, double g, const int32_t* first, const int32_t* mid,
                           int32_t* near_out);     /* oisat_factor_near for a model; not Gaussian: near_out == mid unless forced */
int oisat_set_factor_near(oisat_ctx* h, const int32_t* near, int64_t nb);
/* The factor's shadow (csrc/dense_dag.inc "Shadow"): where an enveloped factorization has a far or a
 * middle block, the task that makes a strictly-lower tile (r, k), first[r] <= k < r, final also stores its two bf16 images,
 * hi = bf16(a) (nearest even) and lo = bf16(a - hi), into a per-handle workspace of 64 KiB per tile, and the two stretches
 * read those instead of converting the fp32 tile in every K-loop.  The factor's bits do not depend on it.  No memory for it:
 * the launch converts in its K-loops, which is not an error.  OISAT_FACTOR_SHADOW in the environment (read at every call):
 * unset or 1 = both stretches read it, 0 = none is made, far / mid = only that stretch reads it; anything else is
 * OISAT_EINVAL of the factorization.
 * oisat_factor_shadow_layout (host only): rowoff_out[r] (int64[nb]) = number of the first tile of block row r, tile (r, k) is
 * number rowoff_out[r] + (k - first[r]); *ntiles_out = sum of r - first[r].  A table that is no envelope is OISAT_EINVAL.
 * oisat_set_factor_shadow_cap: the most bytes the shadow of this handle's later factorizations may take (-1, the default:
 * no limit; 0: never a shadow).
 * oisat_factor_shadow_tile (debugging, tests): the images of tile (r, k) as the LAST factorization on this handle left
 * them, row-major uint16[128 x 128] each; OISAT_EINVAL if that factorization had no shadow or (r, k) is not one of its tiles. */
int oisat_factor_shadow_layout(int nb, const int32_t* first, int64_t* rowoff_out, int64_t* ntiles_out);
int oisat_set_factor_shadow_cap(oisat_ctx* h, int64_t bytes);
int oisat_factor_shadow_tile(oisat_ctx* h, int r, int k, uint16_t* hi_out, uint16_t* lo_out);
int oisat_cov_build_env(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m,
                        double g, float* S, int64_t ld, const int32_t* env_dev);
int oisat_potrf_env(oisat_ctx* h, float* S, int64_t m, int64_t ld, const int32_t* first, const int32_t* env_dev,
                    int* info_host);

/* ---- the build and the factorization of DenseAnalysis.run(): no stores, no sweep the result does not need -----------
 * oisat_cov_build_env_zeroed: oisat_cov_build_env for a caller that KNOWS what the buffer holds.  first = the host
 * table, env_dev = its device copy; zero_first / zero_first_dev (host / device int32[nb], both or neither) = the
 * caller's statement that in block row i every lower tile left of block column zero_first[i] holds exact zeros
 * (NULL: no such statement).  Tiles inside the envelope are evaluated; only the tiles in [zero_first[i], first[i]) are
 * zero-filled; the launch covers those two sets (tile rows x the widest row), not the triangle.  The statement is
 * true after a build and an enveloped task-graph factorization with the table zero_first (neither writes outside the
 * envelope: schedule_out below) as long as nothing else has written to the buffer and ld is the same; a caller that
 * cannot vouch for it passes NULL or calls oisat_cov_build_env, which fills every tile outside the envelope.
 * enveloped_out (optional): 1 = built as described, 0 = OISAT_ENVELOPE=0 made this the dense oisat_cov_build -- the
 * zeros left of the envelope are then correlations: the caller drops its statement.
 * oisat_cov_build_cover (host only): what that launch touches.  from_out[i] = the first block column of block row i
 * it writes (zero-fill up to first[i], evaluation from there), width_out = the most 64 x 64 tiles of one tile row,
 * zero_tiles_out = 128 x 128 tiles that are zero-filled.  Any out pointer may be NULL.
 *
 * oisat_potrf_env_fwd: oisat_potrf_env which also runs the FIRST FORWARD SWEEP of the gain solve of d (device
 * double[m], unchanged until that solve) inside the task-graph launch: row j of the sweep becomes a task when diagonal
 * block j is out and streams its blocks beside the tile tasks, instead of a chain of nb exposed hand-overs behind the
 * launch.  The handle records the forward vector with the factor; the next oisat_gain_solve on this factor with the
 * same d takes it (once), skips its own preparation and forward sweep and starts with the backward sweep -- same
 * arithmetic, same bits.  Any other factorization, oisat_factor_adopt, oisat_potrs or a gain solve of another d drops
 * the record.  Where the factorization does not run as the task graph (OISAT_DAG=0, OISAT_POTRF, under three block rows)
 * or OISAT_FWD_IN_LAUNCH=0 is set (read at every call), this is oisat_potrf_env and the gain solve does all its work.
 * schedule_out (optional): which schedule factored -- OISAT_SCHEDULE_ENV_DAG / _ENV_DAG_FWD (the enveloped task graph,
 * without / with the sweep: nothing outside the envelope was written) or OISAT_SCHEDULE_OTHER (anything else). */
#define OISAT_SCHEDULE_OTHER 0
#define OISAT_SCHEDULE_ENV_DAG 1
#define OISAT_SCHEDULE_ENV_DAG_FWD 2
int oisat_cov_build_env_zeroed(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m,
                               double g, float* S, int64_t ld, const int32_t* first, const int32_t* env_dev,
                               const int32_t* zero_first, const int32_t* zero_first_dev, int* enveloped_out);
int oisat_cov_build_cover(const int32_t* first, const int32_t* zero_first, int64_t nb, int32_t* from_out,
                          int64_t* width_out, int64_t* zero_tiles_out);
int oisat_potrf_env_fwd(oisat_ctx* h, float* S, int64_t m, int64_t ld, const int32_t* first, const int32_t* env_dev,
                        const double* d, int* info_host, int* schedule_out);

/* oisat_trsv_plan (host only): the launch shape of the triangular sweeps of a factor of nb block rows on cu_count CUs.
 * band = the widest block row of an enveloped factor, max over b of (b - first[b]) + 1, or 0 for a dense one.
 * two_tiles_out = 1: every workgroup keeps the row's inverted diagonal block in a second LDS tile (132 KB, one workgroup
 * per CU), staged before the row starts waiting -- chosen when nb <= cu_count or 0 < band <= cu_count / 2; grid_out is
 * then min(nb, cu_count), each workgroup claiming rows by ticket until none is left.  Otherwise one tile and one
 * workgroup per block row.  Either out pointer may be NULL.  In the environment (read at every sweep):
 * OISAT_TRSV_TWO_TILES=0|1 overrides the choice (both are always legal), OISAT_TRSV_MAX_WGS=<n >= 1> caps the grid;
 * anything else in either is OISAT_EINVAL.  Neither changes a bit of any result. */
int oisat_trsv_plan(int64_t nb, int band, int cu_count, int32_t* two_tiles_out, int32_t* grid_out);

/* z <- L^-T L^-1 z  (dev double[m], fp32 factor, double accumulation).  The sweeps' diagonal solves are products with the inverted
 * diagonal blocks, which are float32 (a few 2^-24 of their largest entry from the exact inverses), so ONE pass is as far from
 * the solve on the factor as a float32 substitution.  oisat_potrs therefore corrects once against the factor itself:
 * x1 = M^-1 z, r = z - L (L^T x1) in double, z <- x1 + M^-1 r -- the blocks' error enters squared.  (oisat_gain_solve's passes are
 * single ones: it refines against the float64 S instead.)  Of an enveloped factor only the blocks inside the envelope are read.
 * Cost: two solves (four sweeps) and two O(m^2) passes over the factor by plain kernels, one of them a serial walk down each
 * column -- more than twice a single solve; a diagnostic entry point, not one for a hot path. */
int oisat_potrs(oisat_ctx* h, const float* L, int64_t m, int64_t ld, double* z_inout);

/* r = d - (C.*sig sig^T + diag(var)) z  evaluated in double on the fly (iterative refinement).
 * olat_sorted (may be NULL): dev double[m], latitudes of the observations in degrees, valid only if the
 * observations are stored in ASCENDING latitude order; pairs whose latitudes differ by more than the angle at
 * which the correlation is below 2^-52 are then skipped (one contiguous column range per block of rows). */
int oisat_cov_residual(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m,
                       double g, const double* d, const double* z, double* r_out, const double* olat_sorted);

/* out = r_prev - (C.*sig sig^T + diag(var)) dz: the residual behind a correction z <- z + dz as an update of the one before it.
 * The off-diagonal sums are evaluated in packed fp32 (coordinates, exponential, partial sums of at most 96 terms joined in
 * double), the diagonal term and the subtraction in double: out is within OISAT_RESID_UPDATE_C |r_prev| (2-norm) of the float64
 * value wherever |S dz| is of the order of |r_prev|, which is what a correction of the refinement gives.  Gaussian only, and only
 * where the residual takes compact blocks of rows (the covariance's 2^-64 chord at most 0.5 on the unit sphere: L <= 340 km on
 * the Earth -- 2^-64 is the chord that rule was measured with and keeps, although the sums themselves are cut at 2^-52);
 * OISAT_EINVAL otherwise.  olat_sorted is required; the blocks come from oisat_set_obs_blocks as for
 * oisat_cov_residual (one-shot; without a list: 64 consecutive latitudes).  out must not alias r_prev or dz.  Same inputs,
 * same bits. */
#define OISAT_RESID_UPDATE_C (1.0 / 1024.0)
int oisat_cov_residual_update(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m,
                              double g, const double* r_prev, const double* dz, double* out, const double* olat_sorted);

/* Solve (H B H^T + R) z = d with the fp32 factor as a preconditioner: z = M^-1 d, then at most `refine` rounds of
 * { r = d - S z in float64; stop if |r| <= tol |d|; z += M^-1 r }.  The stopping test runs on the device (the launches of
 * the rounds after convergence return at once; nothing waits for the host).  tol: oisat_set_refine_tol, default 1e-6
 * (the increment is K r away from the exact one and |K| <= 1: fields within 1e-6 |d|); 0 = always run every round.
 * resid_host (may be NULL): relative residual norms before each round and after the last, refine+1 entries; rounds that
 * were not run repeat the last computed value.  Synchronises only when resid_host is given.
 * A residual behind a correction is first formed as oisat_cov_residual_update forms it (Gaussian, compact blocks, tol > 0):
 * t with | |t| - |r| | <= c |r_prev|, c = OISAT_RESID_UPDATE_C.  If |t| + c |r_prev| <= tol |d| -- which proves |r| <= tol |d| --
 * the solve stops there and the norm reported for that round is |t|, within c |previous residual| of the float64 value;
 * otherwise the float64 residual is evaluated and decides, as for every other model and form.  z never depends on t.
 * OISAT_RESID_UPDATE=0 in the environment (read at every call) switches the update form off. */
int oisat_gain_solve(oisat_ctx* h, const float* L, const double* oxyz, const double* osig, const double* ovar,
                     int64_t m, int64_t ld, double g, const double* d, int refine, double* z_out,
                     double* resid_host, const double* olat_sorted /* as for oisat_cov_residual; may be NULL */);

/* inc_i = sig_i * sum_a C(i,a) osig_a z_a  (= row i of B H^T times z);  xa = xb + inc.
 * gxyz: dev double[3*n]; gsig: dev double[n]; z: dev double[m].  xb/xa/inc of `dtype`
 * (either of xa, inc may be NULL).  glat (dev double[n], degrees) and olat_sorted (as for oisat_cov_residual)
 * enable the latitude window: a block of cells only visits the observations within its latitude span +/- the
 * cut-off angle.  Either may be NULL: every pair is evaluated. */
int oisat_apply_increment(oisat_ctx* h, int dtype, const double* gxyz, const double* gsig, int64_t n,
                          const double* oxyz, const double* osig, const double* z, int64_t m, double g,
                          const void* xb, void* xa, void* inc, const double* glat, const double* olat_sorted);

/* The same for cells that form a regular ny x nx grid (row-major, cell = y * nx + x): the kernel then takes compact 32-wide
 * PATCHES of cells per workgroup instead of runs of consecutive cells, gives each patch a bounding sphere and skips the
 * observations of the latitude window that lie beyond the covariance's reach (2^-52) of that sphere -- on a 0.25 deg grid at
 * L = 300 km most of what the latitude window keeps: a polar cap's cells no longer visit the observations on the other
 * side of the pole.  Same sums over the same observations in the same order (terms below 2^-52 of a term left out). */
int oisat_apply_increment_grid(oisat_ctx* h, int dtype, const double* gxyz, const double* gsig, int64_t ny, int64_t nx,
                               const double* oxyz, const double* osig, const double* z, int64_t m, double g,
                               const void* xb, void* xa, void* inc, const double* glat, const double* olat_sorted);

/* oisat_gain_solve followed by oisat_apply_increment_grid of its z, as ONE call that takes the increment off the end of the solve.
 * The increment is linear in z: behind the first solve the call snapshots z0 and runs its float64 increment inc0 into a double
 * scratch field on a stream of the handle's own (lowest priority; waits and is waited for by events), underneath the first
 * residual and the correction's sweeps, which are bound by their hand-overs and leave the vector units idle.  Behind the last
 * round the fields are written once: T(inc0 + delta), T(xb + inc0 + delta) with delta = B H^T (z - z0) as oisat_increment_update
 * forms it, one rounding to T.  Where the refinement converged at the first residual (z = z0) nothing is summed: the bits of
 * oisat_apply_increment_grid.  GUARD, on the device: delta in fp32 is only as good as z - z0 is small, so the update form applies
 * where |r_0| <= OISAT_INC_UPDATE_T |d| (2^-15: the largest power of two t with e t <= 2^-27 for e = 1.69e-4, the largest relative
 * max-norm error of delta measured on four 100 000-observation months); a solve above that gets the float64 increment of its final z,
 * the arithmetic and bits of oisat_apply_increment_grid (of the two launches one returns at once).  z_out and resid_host are oisat_gain_solve's, bit for bit.
 * Gaussian only, 1 <= refine <= 8; OISAT_EINVAL otherwise.  While the side launch is in flight the correction's sweeps take the
 * shape of oisat_trsv_plan_overlap.  With profiling on (oisat_prof_enable) the side launch runs on the handle's stream instead:
 * same kernels, serial, same bits.  The call returns with the side stream joined (no host synchronisation): everything it leaves
 * is ordered behind the handle's stream.  oisat_set_obs_blocks and the forward vector of oisat_potrf_env_fwd are taken as by
 * oisat_gain_solve. */
#define OISAT_INC_UPDATE_T (1.0 / 32768.0)
int oisat_gain_solve_fields(oisat_ctx* h, const float* L, const double* oxyz, const double* osig, const double* ovar,
                            int64_t m, int64_t ld, double g, const double* d, int refine, double* z_out,
                            double* resid_host, const double* olat_sorted, int dtype, const double* gxyz, const double* gsig,
                            int64_t ny, int64_t nx, const void* xb, void* xa, void* inc, const double* glat);

/* The update alone: inc = T(inc0 + delta), xa = T(xb + inc0 + delta), delta_i = sig_i sum_a C(i,a) osig_a (z - z0)_a over the
 * ny x nx grid (row-major).  inc0: dev double[ny * nx] (the float64 increment of z0); z - z0 is taken in double, every pair in
 * packed fp32 (coordinates, exponential, partial sums of 16 terms joined in double), pairs below 2^-20 left out: delta is good
 * to about four digits of its largest entry.  Gaussian only.  Same inputs, same bits. */
int oisat_increment_update(oisat_ctx* h, int dtype, const double* gxyz, const double* gsig, int64_t ny, int64_t nx,
                           const double* oxyz, const double* osig, const double* z, const double* z0, int64_t m, double g,
                           const void* xb, void* xa, void* inc, const double* inc0, const double* glat, const double* olat_sorted);

/* Host only.  oisat_trsv_plan_overlap: the sweeps' shape while the side stream's increment is in flight -- oisat_trsv_plan's, with
 * a two-tile sweep over a band of at most 128 block rows capped at 128 workgroups (one such workgroup leaves a CU room for one
 * increment workgroup instead of five).  oisat_inc_overlap_plan: *use_out = 1 where DenseAnalysis.run takes
 * oisat_gain_solve_fields: one system, Gaussian, refine >= 1, fields wanted, no drift, and at least 256 block rows (the two hidden
 * sweeps must outlast the update's cost); OISAT_INC_OVERLAP=0 in the environment (read at every call): nowhere, =1: wherever it
 * is legal whatever the size; anything else is OISAT_EINVAL. */
int oisat_trsv_plan_overlap(int64_t nb, int band, int cu_count, int32_t* two_tiles_out, int32_t* grid_out);
int oisat_inc_overlap_plan(int64_t nb, int nsys, int corr_kind, int refine, int fields, int drift, int32_t* use_out);

/* perm: dev int32[m], a permutation of 0 .. m-1 that lists the observations (indices into the ascending-latitude order
 * they are stored in) along a space-filling curve, so that 64 consecutive entries are neighbours in space.  The float64
 * residual of the gain solves that follow on this handle for systems of exactly m observations (oisat_gain_solve,
 * oisat_cov_residual) then takes its blocks of 64 rows from this list: a block has a small bounding sphere, and of the
 * latitude window's observations only those within the covariance's reach (2^-52) of it are visited -- the residual's rows
 * are otherwise 64 consecutive LATITUDES, all around the globe.  Same terms per row, staged in the same (latitude) order; a row
 * adds them as four column phases of the list that survives its block's cull, so another list groups the same terms
 * differently: residuals agree to rounding between lists, not to the bit (z of a refined solve: ~1e-15 of its largest entry
 * measured between the identity, the reversal and a Morton order).  NULL / m = 0 clears.
 * ONE-SHOT: the next oisat_gain_solve / oisat_cov_residual call on the handle takes the list (if its m matches) and the handle
 * forgets it, whatever that call returns -- perm must stay valid until that call's work has run, and is never read after. */
int oisat_set_obs_blocks(oisat_ctx* h, const int32_t* perm, int64_t m);

/* X <- X L^-T for nrows (multiple of 128) extra rows, X: dev float[nrows][ldx], ldx >= roundup(m,128).
 * Same MFMA GEMMs as the factorization (block forward substitution with the inverted diagonal blocks).
 * Must follow oisat_potrf of this L. */
int oisat_trsm_rows(oisat_ctx* h, const float* L, int64_t m, int64_t ld, float* X, int64_t nrows, int64_t ldx);

/* Posterior error sqrt(diag(B - B H^T S^-1 H B)) for grid cells [i0, i1):
 * err_i^2 = sig_i^2 - || L^-1 (H B)_{:,i} ||^2 -- rows of (H B)^T are generated on the device in chunks of
 * chunk_rows cells (<= 0: 4096), pushed through oisat_trsm_rows and reduced.  n*m^2 flop: meant for
 * regional / tiled analyses.  Generalises sqrt(Sb) of optimal_interpolation.py:29,:52.  err: dev float[i1-i0]. */
int oisat_posterior_error(oisat_ctx* h, const float* L, int64_t m, int64_t ld, const double* gxyz,
                          const double* gsig, int64_t n, int64_t i0, int64_t i1, const double* oxyz,
                          const double* osig, double g, int64_t chunk_rows, float* err);

/* diag(K H) at the observations: ak_a = 1 - R_aa (S^-1)_aa, (S^-1)_aa = || row a of L^-T ||^2
 * (the dense counterpart of AK = 1 - Sb/(Sa*reg), optimal_interpolation.py:31).  ak_out: dev double[m]. */
int oisat_gain_diag(oisat_ctx* h, const float* L, int64_t m, int64_t ld, const double* ovar, int64_t chunk_rows,
                    double* ak_out);

/* ---- randomized analysis error and averaging kernel ----------------------------------------
 * With S = L L^T, w a vector of independent +-1 entries and u = L^-T w, E[u u^T] = S^-1.  Hence, from K probes u_k,
 *   q_i = g_i^T S^-1 g_i = E[(g_i^T u)^2]   (g_i = row i of B H^T; the analysis error variance is sig_i^2 - q_i)
 *   (S^-1)_aa = E[u_a^2]                     (oisat_gain_diag's ak_a = 1 - R_aa (S^-1)_aa)
 * as sample means whose standard errors come from the fourth moments: the four calls below produce the probes and the
 * sums of squares and of fourth powers; the caller (oisatgmi/dense.py: posterior_error_mc) forms means and errors.
 * All device calls are asynchronous on the handle's stream and use no workspace.
 *
 * oisat_probe_sign (host only): *sign_out = +1.0f or -1.0f, a counter-based hash of (seed, probe, column) -- splitmix64's
 * finaliser applied three times, mix(mix(mix(seed) ^ probe) ^ column), top bit -- the same function on host and device.
 * oisat_probe_fill: X dev float[nrows][ldx], ldx >= roundup(m,128): X[r][a] = oisat_probe_sign(seed, first_probe + r, a) for
 * a < m, exact zeros in the columns m..ldx.  first_probe >= 0, nrows > 0.
 *
 * oisat_trsm_rows_bwd: X <- X L^-1 for nrows (multiple of 128) rows, i.e. row r becomes (L^-T x_r)^T: the backward
 * counterpart of oisat_trsm_rows, same arguments and checks; must follow a factorization of this L on this handle
 * (oisat_potrf, oisat_potrf_env / _fwd, oisat_factor_adopt).  Block columns j = nb-1 .. 0, one launch each: the workgroup
 * of block column k < j applies X_k -= X_j L_jk (128 x 128 x 128 on v_mfma_f32_32x32x2_f32, L_jk read as it lies), the one of
 * k = j-1 then multiplies by the inverted diagonal block and so finishes the next column.  Stream order is the only
 * dependency and one workgroup writes a tile per launch: the bits do not depend on timing.  On an enveloped factor only
 * the blocks first[j] <= k < j are visited (the handle keeps a host copy of first[] with the factor; it is dropped where
 * the envelope is forgotten) and nothing outside the envelope is read.  The padding rows of L are identity: columns
 * m..mp of X pass through unchanged.
 *
 * oisat_probe_spread: t_ik = gsig_i sum_a C(i,a) osig_a U[k][a] under the handle's correlation model, U dev
 * float[nprobe][ldu] (ldu >= m); sum2_out[i] (+)= sum_k t_ik^2, sum4_out[i] (+)= sum_k t_ik^4, dev double[n]; accumulate = 0
 * overwrites.  nx > 0: the cells are an ny x nx grid taken in 32 x 8 patches (oisat_apply_increment_grid); nx = 0: ny
 * consecutive cells in runs of 256 (oisat_apply_increment).  glat / olat_sorted (both or the pair counts as NULL) enable the
 * latitude window and the bounding-sphere cull at the library's 2^-52 chord; NULL: every pair is evaluated.  |p - q|^2 is
 * formed in double, the correlation, the products and the per-probe sums in fp32, the squares and fourth powers are added
 * in double.  nprobe a multiple of 32 with 32 <= nprobe <= 4096, anything else is OISAT_EINVAL.
 *
 * oisat_probe_diag: per observation a < m, sum2_out[a] (+)= sum_k U[k][a]^2, sum4_out[a] (+)= sum_k U[k][a]^4 (double sums
 * in the order of k), dev double[m]; nprobe >= 1. */
int oisat_probe_sign(uint64_t seed, int64_t probe, int64_t column, float* sign_out);
int oisat_probe_fill(oisat_ctx* h, uint64_t seed, int64_t first_probe, float* X, int64_t nrows, int64_t ldx, int64_t m);
int oisat_trsm_rows_bwd(oisat_ctx* h, const float* L, int64_t m, int64_t ld, float* X, int64_t nrows, int64_t ldx);
int oisat_probe_spread(oisat_ctx* h, const double* gxyz, const double* gsig, int64_t ny, int64_t nx, const double* oxyz,
                       const double* osig, const float* U, int64_t nprobe, int64_t ldu, int64_t m, double g,
                       const double* glat, const double* olat_sorted, int accumulate, double* sum2_out, double* sum4_out);
int oisat_probe_diag(oisat_ctx* h, const float* U, int64_t nprobe, int64_t ldu, int64_t m, int accumulate,
                     double* sum2_out, double* sum4_out);

/* ---- analysis error of linear functionals: regional means --------------------------------------
 * For K functionals W (K x n, a row = weights over cells) the analysis error covariance is
 *   A_W = W B W^T - G^T S^-1 G,   G = H B W^T (m x K),   S = H B H^T + R,
 * K refined gain solves through the factor (oisat_gain_solve) and two pair sums, G and T = B W^T; the caller
 * (oisatgmi/dense.py: functional_covariance) forms prior = W T^T and the reduction G^T Y + R^T Y, R = G - S Y.
 * Both device calls are asynchronous on the handle's stream and use no workspace.
 *
 * oisat_functional_gather: out[k][p] = psig_p sum_j C(p, j) ssig_j W[k][j], k < nfun, p < npts, j < nsrc, under the handle's
 * correlation model.  pxyz / sxyz: dev double[3 * npts] / [3 * nsrc], unit vectors x | y | z; psig, ssig: dev double[npts] /
 * [nsrc]; W: dev double[nfun][ldw], ldw >= nsrc; out: dev double[nfun][ldo], ldo >= npts, columns npts..ldo are not written.
 * The sources must be stored in ASCENDING latitude when slat_sorted is given.  plat / slat_sorted (degrees; both or the pair
 * counts as NULL) enable the latitude window and the bounding-sphere cull at the library's 2^-52 chord per run of 256
 * consecutive targets: the terms left out are below 2^-52 of a full term; NULL: every pair is evaluated.  Float64 throughout:
 * |p - q|^2 from the double coordinates, the correlation that oisat_corr_eval evaluates, one fused multiply-add per pair and
 * functional; no fp32 tier.  The sums run in source order; same inputs, same bits.  1 <= nfun <= 64, npts >= 1,
 * 1 <= nsrc < 2^31, anything else is OISAT_EINVAL with nothing launched.
 *
 * oisat_rows_dot: out[k][l] = sum_p A[k][p] B[l][p] in double, A: dev double[na][lda], B: dev double[nb][ldb], lda, ldb >= len,
 * out: dev double[na][nb] (dense).  1 <= na, nb <= 64, len >= 1.  The summation tree depends on len alone (thread t of 256
 * adds p = t, t + 256, ..; lanes by butterfly, waves as (0 + 1) + (2 + 3)): same inputs, same bits on any device. */
int oisat_functional_gather(oisat_ctx* h, const double* pxyz, const double* psig, const double* plat, int64_t npts,
                            const double* sxyz, const double* ssig, const double* slat_sorted, int64_t nsrc,
                            const double* W, int64_t nfun, int64_t ldw, double g, double* out, int64_t ldo);
int oisat_rows_dot(oisat_ctx* h, const double* A, int64_t lda, int64_t na, const double* B, int64_t ldb, int64_t nb,
                   int64_t len, double* out);

/* ---- posterior ensembles by Matheron's rule (csrc/dense_ensemble.hip) -----------------------------
 * A member is a draw from N(x_a, A), A = B - B H^T S^-1 H B:
 *   delta_k = xi_k - B H^T S^-1 (H xi_k + eps_k),   xi_k ~ N(0, B),  eps_k ~ N(0, R),
 * with the prior draw a random-feature field of F frequencies from the correlation's spectral measure in R^3.  The library
 * draws nothing: frequencies, phases and noise are arguments (oisatgmi/dense.py: ensemble_draws, posterior_ensemble), and the
 * solve in the middle is oisat_trsm_rows then oisat_trsm_rows_bwd on the panel.  Both calls are asynchronous on the handle's
 * stream and use no workspace; no workgroup waits for another; same inputs, same bits.
 *
 * oisat_field_sample: out[k][p] = scale_p sqrt(2 / F) sum_{f < F} cos 2 pi (omega_kf . x_p + phi_kf) + sqrt(nscale_p) noise[k][p],
 * k < nmember, p < npts.  pxyz: dev double[3 * npts], unit vectors x | y | z; omega: dev double[nmember][3][nfeature] -- per
 * member the x components of its F frequencies, then y, then z -- in TURNS per unit chord (angular frequency / 2 pi); phase: dev
 * double[nmember][nfeature] in turns; scale: dev double[npts] or NULL (= 1); noise: dev float[nmember][ld] with nscale: dev
 * double[npts], both given or both NULL (no second term); out: dev float[nmember][ld], ld >= npts, the columns npts..ld are
 * written as exact zeros (the row sweeps pass them through).  Per point and feature the phase is formed in double (three fused
 * multiply-adds onto phi, x first) and reduced by its nearest integer in double; the remainder is narrowed to float, its
 * cosine is an fp32 one and the F cosines are added in fp32 in the order of f; the closing expression is double, rounded
 * once.  nfeature >= 1, 1 <= nmember <= 65535, npts >= 1, anything else is OISAT_EINVAL with nothing launched.
 *
 * oisat_member_spread: P[k][i] <- P[k][i] - gsig_i sum_a C(i,a) osig_a U[k][a] in place, under the handle's correlation model,
 * P: dev float[nmember][ldp] (ldp >= the number of cells), U: dev float[nmember][ldu] (ldu >= m); sum2_out[i] (+)= sum_k P[k][i]^2
 * and sum4_out[i] (+)= sum_k P[k][i]^4 of the UPDATED values, dev double[n]; accumulate = 0 overwrites.  oisat_probe_spread with
 * the per-vector sum stored instead of squared -- one kernel, csrc/dense_spread.inc -- hence its patches (nx > 0: 32 x 8; nx = 0:
 * runs of 256), its latitude window and cull (glat / olat_sorted, both or the pair counts as NULL), its number formats (the sum
 * over a in fp32; the subtraction in double, rounded once to the float that is stored and squared) and its rule for nmember: a
 * multiple of 32 with 32 <= nmember <= 4096, anything else is OISAT_EINVAL. */
int oisat_field_sample(oisat_ctx* h, const double* pxyz, int64_t npts, const double* scale, const double* omega,
                       const double* phase, int64_t nfeature, int64_t nmember, const float* noise, const double* nscale,
                       float* out, int64_t ld);
int oisat_member_spread(oisat_ctx* h, const double* gxyz, const double* gsig, int64_t ny, int64_t nx, const double* oxyz,
                        const double* osig, const float* U, int64_t nmember, int64_t ldu, int64_t m, double g,
                        const double* glat, const double* olat_sorted, float* P, int64_t ldp, int accumulate,
                        double* sum2_out, double* sum4_out);

/* The likelihood of the innovations under the analysis' own model (csrc/dense_likelihood.hip):
 * -2 ln p(d) = m ln 2 pi + log det S + d^T S^-1 d with S = H B H^T + R = L L^T.  chi^2 = d^T z and |d|^2 are oisat_rows_dot with
 * na = nb = 1; the log-determinant is
 *
 * oisat_factor_logdet: out[0] = 2 sum_{a < m} log((double)L[a * ld + a]), out[1] = the smallest L[a * ld + a], a < m, as a double.
 * L: dev float[>= m][ld], the factor any factorization of this library left in S (oisat_potrf, oisat_potrf_env,
 * oisat_potrf_env_fwd, a member of a batch): they all keep the diagonal of L on the diagonal of S.  out: dev double[2].  Only
 * the m diagonal entries are read -- not the identity padding m..roundup(m, 128), not a gutter beyond it.  If any of them is
 * <= 0, infinite or NaN, out[0] is NaN (out[1] is still the smallest one that is a number, +inf if none is); nothing is added to the handle's
 * status words.  Float64 throughout: the logarithm of the widened float, then a fixed tree -- one workgroup of 1024 threads,
 * thread t takes a = t, t + 1024, .. into four partial sums by turn, joined (0 + 1) + (2 + 3); lanes by butterfly; the 16 waves
 * pairwise, neighbours first -- which depends on m alone: same inputs, same bits on any device.  Asynchronous on the handle's
 * stream, no workspace.  NULL h, L or out, m < 1 or ld < roundup(m, 128): OISAT_EINVAL, nothing launched, out untouched. */
int oisat_factor_logdet(oisat_ctx* h, const float* L, int64_t m, int64_t ld, double* out);

/* ---- a drift of the innovations: universal kriging (csrc/dense_drift.hip) -------------------------
 * d = F beta + e, e ~ N(0, S), S = H B H^T + R, beta unknown with a flat prior, F = p smooth basis functions at the observations:
 *   beta = M^-1 F^T S^-1 d,  M = F^T S^-1 F,  z' = S^-1 (d - F beta),  x_a = x_b + B H^T z' + f(x)^T beta,
 * and the unknown beta adds q^T M^-1 q to a cell's analysis error variance, q = f(x) - F^T S^-1 H B e_x.  The library evaluates the
 * basis, solves S [z_d, Y_F] = [d, F] as ONE block through the factor a run left behind, and applies beta; the p x p system is
 * the caller's (oisatgmi/dense.py: DenseAnalysis.run(drift=...)), with M and b = F^T z_d from oisat_rows_dot.  All five calls are
 * asynchronous on the handle's stream (oisat_gain_solve_multi: unless resid_host is given) and no workgroup waits for another.
 *
 * oisat_drift_basis: out[j][i] = f_j(p_i), j < p = (degree + 1)^2, i < npts; pxyz: dev double[3 * npts], unit vectors x | y | z;
 * out: dev double[p][ld], ld >= npts, the columns npts..ld are written as zeros.  degree = 0 .. 3.  The functions are the real
 * harmonics up to `degree` as polynomials of (x, y, z), unnormalised, in this order and evaluated exactly as written -- float64,
 * one rounding per operation, no fused multiply-add, with xx = x*x, yy = y*y, zz = z*z, xy = x*y, t = 5*zz formed once:
 *   degree 0:  1
 *   degree 1:  x,  y,  z
 *   degree 2:  xy,  y*z,  z*x,  xx - yy,  3*zz - 1
 *   degree 3:  z*(t - 3),  x*(t - 1),  y*(t - 1),  z*(xx - yy),  xy*z,  x*(xx - 3*yy),  y*(3*xx - yy)
 * so the same inputs give the same bits, on the device and in a NumPy restatement.  NULL h, pxyz or out, degree outside 0..3,
 * npts < 1 or ld < npts: OISAT_EINVAL with nothing launched.
 *
 * oisat_cov_residual_multi: R[k] = D[k] - (C.*sig sig^T + diag(var)) Z[k] for k < nrhs, 1 <= nrhs <= 17, in float64 from the
 * coordinates under the handle's correlation model (all three), in ONE pass over the pairs: each correlation value is formed
 * once and enters nrhs fused multiply-adds.  D, Z, R_out: dev double[nrhs][ld], ld >= m, the columns m..ld are neither read nor
 * written.  olat_sorted: as for oisat_cov_residual (the same latitude window); the one-shot block list of oisat_set_obs_blocks is
 * taken as oisat_cov_residual takes it (used where that call would use it: a window exists and the compact blocks pay), the cull
 * then being per block of 64 rows at the 2^-52 chord -- the terms left out are below 2^-52 of a full term.  A row's sum runs over
 * the candidates in latitude order, four column phases (every fourth surviving candidate of each run of 64) joined as
 * ((0 + 1) + 2) + 3: same inputs, same bits; the columns do not influence each other.  No fp32 tier.  R_out must not overlap D
 * or Z; that, nrhs outside 1..17, m < 1, m >= 2^31, ld < m or a NULL pointer is OISAT_EINVAL with nothing launched.
 *
 * oisat_gain_solve_multi: oisat_gain_solve for a block of right-hand sides D (dev double[nrhs][ld]) into Z_out (same shape;
 * must not overlap D): Z[k] = M^-1 d_k, then at most `refine` (0..8) rounds of { R = D - S Z by oisat_cov_residual_multi; a
 * column with |r_k| <= tol |d_k| is converged (tol: oisat_set_refine_tol) and takes ZERO corrections from then on; Z += M^-1 R }.
 * M^-1 is oisat_trsm_rows then oisat_trsm_rows_bwd on an fp32 panel of 128 rows (the rows nrhs..128 are zeros), i.e. GEMMs on
 * the matrix cores over the whole lower triangle of the factor; Z is accumulated in double.  Narrowing to fp32 needs a scale per
 * column: every right-hand side and every residual is divided by |d_k| on the way into the panel and the correction multiplied
 * by |d_k| on the way out, so a column of norm 1e-25 or 1e+45 (both tested) neither underflows nor overflows, and a column of zeros gives
 * zeros.  The test runs on the device.  A column still above tol behind the last allowed correction adds one to
 * OISAT_STATUS_UNCONVERGED, as a single solve does; refine = 0 forms no residual (unless resid_host asks) and flags nothing.
 * resid_host (may be NULL): (refine + 1) x nrhs relative norms |r_k| / |d_k|, [round][column]; rounds a column did not run repeat
 * its last value.  Without resid_host the call enqueues every round and returns; with it the call synchronises after each
 * check and stops enqueuing once every column has converged (the results are the same bits either way: a converged column's
 * corrections are exact zeros).  L, m, ldl: the factor of the last factorization on this handle, as for oisat_gain_solve; the
 * block list of oisat_set_obs_blocks is taken once and serves every round.  Workspace: the handle's, (128 x roundup(m, 128))
 * floats + nrhs x ld doubles, grown on first use (not sized by oisat_dense_reserve).
 *
 * oisat_drift_apply: x_i += sum_j beta_j f_j(x_i) and inc_i += the same, i < n; gxyz: dev double[3 * n]; beta: dev double[p];
 * x_inout, inc_inout: dev `dtype`[n], either may be NULL (not both).  The sum is formed in double (fused multiply-adds in the
 * order of j), added to the widened value in double and rounded once to `dtype`.
 *
 * oisat_drift_quadform: var_out[i] = q_i^T Minv q_i, q_i[j] = f_j(x_i) - Q[j][i], i < n; Q: dev double[p][ldq], ldq >= n; Minv:
 * dev double[p][p], row-major; var_out: dev double[n].  The basis is evaluated inside the kernel by the expressions above;
 * t_j = sum_k Minv[j][k] q_k then sum_j q_j t_j, fused multiply-adds in ascending order. */
int oisat_drift_basis(oisat_ctx* h, const double* pxyz, int64_t npts, int degree, double* out, int64_t ld);
int oisat_cov_residual_multi(oisat_ctx* h, const double* oxyz, const double* osig, const double* ovar, int64_t m, double g,
                             const double* D, const double* Z, double* R_out, int64_t nrhs, int64_t ld,
                             const double* olat_sorted);
int oisat_gain_solve_multi(oisat_ctx* h, const float* L, const double* oxyz, const double* osig, const double* ovar,
                           int64_t m, int64_t ldl, double g, const double* D, int64_t nrhs, int64_t ld, int refine,
                           double* Z_out, double* resid_host, const double* olat_sorted);
int oisat_drift_apply(oisat_ctx* h, int dtype, const double* gxyz, int64_t n, int degree, const double* beta,
                      void* x_inout, void* inc_inout);
int oisat_drift_quadform(oisat_ctx* h, const double* gxyz, int64_t n, int degree, const double* Q, int64_t ldq,
                         const double* Minv, double* var_out);

/* The ticket list of a task-graph launch over nsys systems of block_rows[s] block rows (largest first), as the library would
 * build it -- host only, no device: int32 quadruples (kind, system, i, j) with kind 0 = chain of `system` (i = first row of its
 * trace stamps), 1 = tile task T(i, j), 2 = SUB(j) (tile (j+1, j)), 3 = PRE(j) (tile (j, j)).  (The solve tasks of
 * oisat_batch_analyse are not tickets: they enter the launch's ready queue when their input is complete.)  wave <= 0: the
 * default (eight systems per wave behind wave 0).  capacity = 0 just counts.  max_wave_chains_out (may be NULL): the chain
 * tickets that can be resident at one time (the largest wave's and the next one's) -- a launch is only made when four times
 * that many workgroups are resident (each chain holds one and waits for tasks that the others must draw); otherwise the
 * factorization keeps the lock-step recursion.  For tests of the scheduling rule (every input of a task carries a lower
 * ticket, or is its system's chain) and of that bound. */
int oisat_dag_task_order(int nsys, const int32_t* block_rows, int wave, int32_t* tasks_out, int64_t capacity,
                         int64_t* ntasks_out, int32_t* reserve_out, int32_t* max_wave_chains_out);
/* ... and of the ENVELOPED launch of one system of nb <= 1024 block rows (oisat_potrf_env): first = its envelope, far = its
 * far stretch (oisat_factor_far) or NULL.  A bulk task's first word is kind | k0 << 8 | kfar << 18 (ten bits each): its
 * K-loop runs over the block columns k0 = first[i] .. kend - 1 (kend = j, PRE: j - 1), the blocks k0 .. kfar - 1 of it on
 * the bf16 pipe, k0 <= kfar = clamp(far[i]) <= kend.  Profiling aid, this query only: OISAT_DAG_ORDER_LEAD_FAR = a number in
 * [0, 1) gives the order a far list would have at that ticket lead (tools/dag_sched_model.py); anything else is OISAT_EINVAL.
 * No launch reads it. */
int oisat_dag_task_order_env(int nb, const int32_t* first, const int32_t* far, int32_t* tasks_out, int64_t capacity,
                             int64_t* ntasks_out);

/* Schedule of the factorizations this handle runs from now on (oisat_potrf, batches made by oisat_batch_create): 1 = the
 * task graph (ONE persistent launch of left-looking tile tasks, csrc/dense_dag.inc) wherever it applies, 0 = the recursion
 * (one launch per node, lock-step over a batch), -1 (default) = by size: the task graph from three block rows up, unless the
 * environment says otherwise (OISAT_DAG=0 | 1).  A caller that overlaps several batches on one GPU -- twelve months as two
 * lock-step groups -- switches the task graph off for them: a persistent launch holds every workgroup slot until it is done. */
int oisat_set_task_graph(oisat_ctx* h, int mode);

/* How a handle's batched factorization shares the GPU with other handles' work that runs at the same time (several
 * groups of systems factored side by side, oisatgmi/dense.py BatchedFactor): wave_prio 0..3 = s_setprio of its kernels'
 * waves -- where waves of two groups sit on one SIMD the arbiter serves the higher one first, so the group with the
 * longest dependent chain (the polar caps of a localised month) is not slowed by the other group's bulk GEMMs;
 * gemm_wg_per_cu 1 | 2 (0 = default 2) = workgroups per CU of its persistent GEMM launches, 1 leaves a slot on every CU
 * to the other group.  Results do not depend on either. */
int oisat_set_share(oisat_ctx* h, int wave_prio, int gemm_wg_per_cu);

/* Relative residual |d - S z| / |d| at which oisat_gain_solve stops refining on this handle (default 1e-6; 0: never, short of
 * a residual that is exactly zero -- a system of one observation behind a correction or two). */
int oisat_set_refine_tol(oisat_ctx* h, double tol);

/* ---- batched factorization: many independent systems in lock-step ---------------------------------------------------
 * The tiles of a localised analysis (and the months of a batch) are small systems -- 4,000-18,000 observations -- whose
 * factorization is a chain of ~3 dependent launches per 128 columns, most of them far too small to fill 256 CUs.
 * oisat_batch_potrf advances all matrices of a batch through the SAME recursion at once: every launch covers every
 * matrix the step applies to (blockIdx.y = matrix), so the chain is paid once per batch and the launches are large.
 * The recursion tree is that of the LARGEST matrix of the batch: its factor is bit-identical to oisat_potrf's, the
 * smaller ones see their trailing updates associated differently and agree with oisat_potrf to fp32 rounding.
 *
 * oisat_batch_create: S[i] (dev, m[i] rows padded to roundup(m[i],128), leading dimension ld[i]) and tinv[i] (dev,
 *   roundup(m[i],128)*128 floats: receives the inverted diagonal blocks) for nmat matrices; HOST arrays of device pointers
 *   / sizes, copied.  The batch belongs to handle h and is factored on h's stream.
 * oisat_batch_potrf: pad + factor every matrix in place.  info_host (may be NULL; then failures are left to
 *   oisat_solve_status): int[2] = {first non-positive pivot column (1-based, 0 = none), index of that matrix}; synchronises.
 * oisat_factor_adopt: tell handle h that L (as factored by a batch, or by oisat_potrf on another handle) with inverted
 *   diagonal blocks tinv is "its" factor, so that oisat_gain_solve / oisat_potrs / oisat_trsm_rows / oisat_posterior_error
 *   on h accept it.  The caller orders the streams (oisat_wait_for). */
int oisat_batch_create(oisat_ctx* h, int nmat, float* const* S, const int64_t* m, const int64_t* ld, float* const* tinv,
                       int* batch_id_out);
int oisat_batch_potrf(oisat_ctx* h, int batch_id, int* info_host);

/* The solve phase of a batch in lock-step as well (round 3): after oisat_batch_set_solve has told the batch where every
 * member keeps its observations, innovation, solution, work vectors and grid, oisat_batch_solve enqueues -- on the batch's
 * handle, behind oisat_batch_potrf, no host hand-over -- the gain solve and the increment of ALL members with one launch
 * per step: pad, forward / backward sweep (tickets over (member, block row), rows ascending, so the factors of all systems
 * are streamed level by level), float64 residual, convergence test (per member, oisat_set_refine_tol), at most `refine`
 * corrections, increment.  Per member the arithmetic is that of oisat_gain_solve + oisat_apply_increment(_grid) -- the same bits
 * for the plain solve, for every solve that takes no correction, for a refined solve on compact blocks of rows, and always for
 * the increment of a given z -- with one exception: where the residual runs on latitude rows (no perm for some member, or a
 * correlation length beyond the compact blocks' range) oisat_gain_solve cuts the columns into slices and adds the slices' sums
 * in a second launch, the batched launch does not; the residuals agree to rounding and a z behind a correction differs in its
 * last bits (2.7e-16 of its largest entry measured).  Every array is in the caller's order, whatever order the library keeps
 * the members in; a refused oisat_batch_set_solve / oisat_batch_set_grid leaves the batch as it was.
 * Arrays are indexed like those of oisat_batch_create.  work[i]: dev double[2 * roundup(m_i, 128)]; state[i]: dev, 256
 * zeroed bytes; observations in ascending latitude (olat[i]); xa[i] | inc[i]: where the analysis and the increment of
 * member i go (dtype of oisat_batch_solve). */
int oisat_batch_set_solve(oisat_ctx* h, int batch_id, int nmat, const double* const* oxyz, const double* const* osig,
                          const double* const* ovar, const double* const* d, const double* const* olat, double* const* z,
                          double* const* work, void* const* state, const double* const* gxyz, const double* const* gsig,
                          const double* const* glat, const int64_t* n, const void* const* xb, void* const* xa,
                          void* const* inc);
/* nx[i]: width of member i's cell grid (its n[i] cells are (n[i] / nx[i]) x nx[i], row-major; 0 = no such shape): the
 * increment of oisat_batch_solve then works like oisat_apply_increment_grid.  perm (may be NULL, entries may be NULL):
 * perm[i] = member i's observations along a space-filling curve, dev int32[m_i] (see oisat_set_obs_blocks): its float64
 * residuals then run on compact blocks of rows.  After oisat_batch_set_solve. */
int oisat_batch_set_grid(oisat_ctx* h, int batch_id, int nmat, const int64_t* nx, const int32_t* const* perm);
int oisat_batch_solve(oisat_ctx* h, int batch_id, int dtype, double g, int refine);
/* oisat_batch_potrf + oisat_batch_solve as ONE task-graph launch: every member's factorization, gain solve (sweeps, float64
 * residuals, convergence test, at most `refine` corrections) and increment are tasks of one persistent launch -- put into its
 * ready queue by the task that completes their input -- so the solves of the systems that are factored first run underneath
 * the factorization of the others instead of behind the whole batch
 * (a localised 720x1440 month: the solve phase was 12 of 62 ms with idle MFMA pipes).  Per member the same arithmetic as the
 * two calls.  Needs oisat_batch_set_solve (and oisat_batch_set_grid) and a batch whose factorization runs as a task graph
 * (oisat_set_task_graph; OISAT_EINVAL otherwise -- use the two calls).  info_host as in oisat_batch_potrf (NULL: unchecked,
 * asynchronous; failures go to oisat_solve_status_ex). */
int oisat_batch_analyse(oisat_ctx* h, int batch_id, int dtype, double g, int refine, int* info_host);
/* *yes_out = 1 if the batch's factorization runs as a task graph (decided at oisat_batch_create: the handle's schedule, the
 * sizes, and whether the chains of its largest wave leave room on the handle's CUs), i.e. whether oisat_batch_analyse applies. */
int oisat_batch_is_task_graph(oisat_ctx* h, int batch_id, int* yes_out);
int oisat_batch_destroy(oisat_ctx* h, int batch_id);
int oisat_factor_adopt(oisat_ctx* h, const float* L, int64_t m, int64_t ld, float* tinv);

/* ---- RCCL over xGMI: the two collectives of the sharded path ---------------------------------
 * The reference runs one scheduler job per month and exchanges nothing (run/job_submitter_sbatch.py:45-68).  One
 * process per GPU, (month x tile) units sharded statically: what is shared is broadcast once (the model grid), finished
 * fields are gathered to the root -- there is no collective on the data path.  librccl is dlopen'ed at the first call
 * (a copy already in the process, e.g. PyTorch's, is reused).  Enqueued on the handle's stream, asynchronous.
 *   oisat_comm_unique_id  on ONE rank: 128 opaque bytes, to be handed to every rank by the launcher (file, env, MPI, ...)
 *   oisat_comm_init       collective over all ranks: joins rank `rank` of `nranks`
 *   oisat_comm_bcast      dev_buf (bytes) of `root` -> every rank's dev_buf, in place
 *   oisat_comm_gather     every rank's `bytes` at send_dev -> recv_dev + r*bytes on `root` (recv_dev ignored elsewhere):
 *                         a gather, not an all-gather -- only the root needs the fields */
int oisat_comm_unique_id(char* id_out, int cap /* >= 128 */);
int oisat_comm_init(oisat_ctx* h, int rank, int nranks, const char* unique_id);
int oisat_comm_bcast(oisat_ctx* h, void* dev_buf, size_t bytes, int root);
int oisat_comm_gather(oisat_ctx* h, const void* send_dev, size_t bytes, void* recv_dev, int root);
int oisat_comm_destroy(oisat_ctx* h);

/* Status of the dense solves enqueued on this handle since the last call with clear != 0 (synchronises the stream; one
 * 36-byte read-back).  oisat_potrf / oisat_gain_solve only report failures when given info_host / resid_host; an
 * unchecked (fully asynchronous) run records them here instead.  out[0 .. nwords-1], nwords <= OISAT_STATUS_WORDS:
 *   OISAT_STATUS_NOTPD_COL          1-based column of the first non-positive pivot of any factorization (0 = none)
 *   OISAT_STATUS_NOTPD_BLOCKS       number of diagonal blocks that met one
 *   OISAT_STATUS_TRSV_TIMEOUTS      triangular-solve workgroups that gave up waiting for a predecessor (their part of z is a
 *                                   NaN fill pattern)
 *   OISAT_STATUS_UNCONVERGED        gain solves (oisat_gain_solve, members of oisat_batch_solve / oisat_batch_analyse) that took
 *                                   every one of their `refine` corrections and whose float64 residual |d - S z| was still above
 *                                   tol |d| behind the last one (oisat_set_refine_tol; tol = 0 and refine = 0 -- the plain
 *                                   solve, no residual is formed -- never count): z is the best
 *                                   iterate, NOT within the tolerance -- the exact gain of optimal_interpolation.py:27 is what
 *                                   the 1e-5 bar is measured against, so a caller must not take such fields for converged ones
 *   OISAT_STATUS_UNCONVERGED_MEMBER the LOWEST caller's index (oisat_batch_create order) among the batch members that ended so
 *                                   since the last clear -- a minimum, whichever member's workgroup reports first, in
 *                                   oisat_batch_solve and oisat_batch_analyse alike; -1 = none, or a single-system solve
 *   OISAT_STATUS_DAG_TIMEOUTS       task-graph factorizations that ended on a time-out (bounded spins): incomplete factors
 * A caller must see zeros in words 0-3 and 5 before it trusts z / the analysis fields. */
enum { OISAT_STATUS_NOTPD_COL = 0, OISAT_STATUS_NOTPD_BLOCKS = 1, OISAT_STATUS_TRSV_TIMEOUTS = 2, OISAT_STATUS_UNCONVERGED = 3,
       OISAT_STATUS_UNCONVERGED_MEMBER = 4, OISAT_STATUS_DAG_TIMEOUTS = 5, OISAT_STATUS_WORDS = 6 };
int oisat_solve_status_ex(oisat_ctx* h, int32_t* out, int nwords, int clear);
/* The round-2 form: three words.  (It clears all six, so trsv_timeouts here also counts unconverged solves and task-graph
 * time-outs: three zeros still mean "trust the fields".)  Any of the three may be NULL. */
int oisat_solve_status(oisat_ctx* h, int* first_notpd_col, int* n_notpd_blocks, int* trsv_timeouts, int clear);

/* Pre-size every internal workspace of the dense path for analyses of up to max_obs observations (and, if
 * diag_chunk_rows > 0, for oisat_posterior_error / oisat_gain_diag with that chunk size), so that no later
 * oisat_potrf / oisat_gain_solve / ... call on this handle allocates or frees device memory. */
int oisat_dense_reserve(oisat_ctx* h, int64_t max_obs, int64_t diag_chunk_rows);

/* ---- the innovations' covariogram (Hollingsworth-Loennberg): what the data say about the correlation length ----------
 * oisat_covariogram: oxyz dev double[3][m] unit vectors, d dev double[m] innovations, w dev double[m] or NULL; u_a = d_a w_a
 * (NULL: u = d; the caller passes 1 / (sig_b sqrt(scale))).  An observation whose u is NaN or +-inf takes part in nothing;
 * *nobs_used_out (host, may be NULL) counts the others.  For every pair a < b of used observations
 *   dx = xa - xb (dy, dz likewise), d2 = dx dx + dy dy + dz dz left to right (no FMA), chord = sqrt(d2),
 *   k = (int64)(chord * (nbins / max_chord))        (the factor computed once on the host in double)
 * and, unless k >= nbins:  count[k] += 1, sum_prod[k] += u_a u_b, sum_chord[k] += chord.
 * count_out / sum_prod_out / sum_chord_out: HOST arrays of nbins.  Synchronises, like oisat_oi_curve.
 * olat_sorted (dev double[m], degrees, or NULL) as for oisat_cov_residual: valid only if the observations are stored in
 * ASCENDING latitude; a block of 256 rows then visits only the columns up to the latitude of its last row plus
 * 2 asin(min(max_chord, 2) / 2).  What is skipped lies beyond max_chord: the outputs are the same bits with and without it.
 * 0 <= m <= 1 << 20 (m = 0 or 1: zeros), 1 <= nbins <= 1024, max_chord > 0 and finite; anything else is OISAT_EINVAL and
 * leaves the outputs untouched.
 * The sums are exact integers, hence independent of the order of the atomics, of the launch shape, of the window and of the
 * order of the observations, bit for bit: with P = m (m - 1) / 2, umax = the largest finite |u| (a device reduction) and e
 * the frexp exponent of umax * umax * (double)P, q_prod = 2^(e - 62) (1 if that product is 0); q_chord = 2^(e_c - 62), e_c the
 * frexp exponent of 2.0 * (double)max(P, 1); either exponent is kept at -1022 or above.  Each term is rounded once, to
 * llrint(term / q) (an exact division, nearest even), the terms are added as int64 (below 2^63 by the choice of q) and a
 * bin's output is (double)sum * q.  So |sum_prod[k] - exact| <= count[k] q_prod / 2 plus the last bit of the result, and
 * likewise sum_chord with q_chord and the chord's own rounding.  umax^2 P must be finite.
 * Workspace: 24.6 KB + 8 m bytes on the handle, grow-only, allocated at the first call that needs it (oisat_dense_reserve
 * does not cover it).
 * oisat_covariogram_quantum (host only): the two quanta by this rule, for tests and callers that bound the error without
 * asking the kernel; m outside 0 .. 1 << 20, umax negative or NaN, or umax^2 P not finite is OISAT_EINVAL. */
int oisat_covariogram(oisat_ctx* h, const double* oxyz, const double* d, const double* w, int64_t m, double max_chord,
                      int nbins, const double* olat_sorted, int64_t* count_out, double* sum_prod_out, double* sum_chord_out,
                      int64_t* nobs_used_out);
int oisat_covariogram_quantum(double umax, int64_t m, double* q_prod_out, double* q_chord_out);

/* ---- buddy sums of the normalised innovations: quality control ahead of the dense analyses ------
 * oisat_buddy_sums: oxyz dev double[3][m] unit vectors, u dev double[m] normalised innovations, n_out dev int32[m], sums_out
 * dev double[3][m] = W[m] | P[m] | Q[m]; every pointer a device pointer.  Enqueued on the handle's stream, does not
 * synchronise, no workspace on the handle.  The correlation model is the handle's (oisat_set_correlation), any of the three.
 * An observation whose u is NaN or +-inf takes part in nothing, and its own outputs are n = 0, W = P = Q = 0 (the
 * covariogram's convention).  For every used a, over the used b != a in ASCENDING b:
 *   dx = xa - xb (dy, dz likewise), d2 = dx dx + dy dy + dz dz left to right (no FMA),
 *   c = C(d2; g) by the library's float64 correlation function (the one behind oisat_corr_eval),
 *   if c >= cmin:  n_a += 1, W_a += c, t = c u_b, P_a += t, Q_a += t u_b.
 * So P / W is the correlation-weighted mean of the buddies' innovations and Q / W - (P / W)^2 their weighted spread.
 * olat_sorted (dev double[m], degrees, or NULL) as for oisat_cov_residual / oisat_covariogram: valid only if the observations
 * are stored in ASCENDING latitude; a block of 256 rows then visits only the columns whose latitude lies within the window
 * angle of its first and last row, 2 asin(chord / 2) of the chord at which C has fallen to cmin (oisat_corr_cut_chord's chord
 * at -log2(cmin) bits, here for any cmin below 1), widened by 1e-9 relative in chord^2 plus 1e-15 / g, and by 1e-9 degrees.
 * Inside the window a pair whose d2 exceeds that widened squared chord is skipped without evaluating C.  Both skip only
 * pairs that fail c >= cmin for certain.
 * Deterministic: a row's four accumulators live in one lane's registers, which takes the columns in ascending order; rows
 * are not split over workgroups; a skipped pair adds nothing.  The outputs are the same bits on every run, and the same bits
 * with and without olat_sorted.  (They do depend on the ORDER of the observations, as any floating-point sum does.)
 * 0 <= m <= 1 << 20 (m = 0: nothing is done; m = 1: zeros), g > 0 and finite, 2^-20 <= cmin < 1, non-NULL oxyz / u / n_out /
 * sums_out where m > 0; anything else is OISAT_EINVAL and writes nothing. */
int oisat_buddy_sums(oisat_ctx* h, const double* oxyz, const double* u, int64_t m, double g, double cmin,
                     const double* olat_sorted, int32_t* n_out, double* sums_out /* W[m] | P[m] | Q[m] */);

/* ---- superobservations: the observations of one box merged into one, ahead of the dense analysis ----
 * BOXES: a reduced latitude-longitude grid of roughly equal area.  nbands = ceil(180 / box_deg) latitude bands; band j covers
 * [lo_j, hi_j) with lo_j = -90 + (double)j box_deg and hi_j = min(-90 + (double)(j + 1) box_deg, 90) (the last band may be
 * short, and it takes latitude 90 itself); mid_j = 0.5 (lo_j + hi_j); the band has
 *   n_j = max(1, llrint(360 cos(mid_j (pi / 180)) / box_deg))          (left to right, pi / 180 one constant)
 * longitude boxes of 360 / n_j degrees starting at longitude 0; offset_j = n_0 + .. + n_(j-1); box id = offset_j + k;
 * nbox = offset_nbands.
 * oisat_superob_boxes (host only, no device call, float64): writes n_out[nbands] (int32) and offset_out[nbands] (int64), HOST
 * arrays of `cap` entries (cap = 0: neither is written, the two counts alone), *nbands_out and *nbox_out (either may be NULL).
 * box_deg finite and in (0, 180], 180 / box_deg <= 1 << 23, and cap = 0 or >= nbands; anything else is OISAT_EINVAL and
 * writes nothing.
 * THE BOX OF AN OBSERVATION, on the device, one rounding per operation and no FMA:
 *   j = min((int64)floor((lat + 90) / box_deg), nbands - 1)
 *   r = lon / 360,  t = r - floor(r)                                   (t in [0, 1]; 1 for a tiny negative lon)
 *   k = min((int64)(t * (double)n_j), n_j - 1),   box = offset_j + k.
 * An observation takes part iff lat, lon, d, sigma_b and var are finite, |lat| <= 90, var > 0 and w = 1 / var is finite; every
 * other observation gets box -1 and adds nothing.  oxyz is not tested: the caller supplies unit vectors, as everywhere else.
 * oisat_superob: olat, olon (degrees), d, sigma_b, var: dev double[m]; oxyz: dev double[3][m] unit vectors; box_n (int32) and
 * box_offset (int64): HOST arrays of nbands, with nbox the table of oisat_superob_boxes(box_deg) -- checked (nbands =
 * ceil(180 / box_deg), every n_j >= 1, the offsets their running sum, nbox its end, nbox <= 1 << 23), because the device
 * indexes the accumulators with it.  box_out: dev int32[m].  count_out: HOST int64[nbox].  sums_out: HOST
 * double[OISAT_SUPEROB_NSUMS][nbox], quantity-major, or NULL: box ids and counts only (oxyz may then be NULL and no quantum is
 * formed).  *nused_out (host, may be NULL): the observations that take part.  Two launches on the handle's stream (the maxima,
 * the sums), then it SYNCHRONISES and copies the results to the host, like oisat_covariogram.  With w = 1 / var, per box:
 *   count += 1, W += w, Q += sqrt(w), D += w d, V += (w d) d, G += w sigma_b, Px += w x, Py += w y, Pz += w z.
 * The sums are exact integers by the covariogram's rule, hence independent of the order of the observations, of the launch
 * shape and of the run, bit for bit.  With wmax, dmax, smax the largest w, |d|, |sigma_b| over the observations that take
 * part (a device reduction), M = (double)max(m, 1), and for a bound b: q(b) = 2^(e - 62), e the frexp exponent of b M (1 if
 * b M = 0; the exponent kept at -1022 or above):
 *   q_W = q(wmax),  q_Q = q(2^ceil(e_w / 2)) with e_w the frexp exponent of wmax (sqrt(w) is below that power of two),
 *   q_D = q(wmax dmax),  q_V = q(wmax dmax dmax),  q_G = q(wmax smax),  q_P = q(2 wmax) for all three components
 * (products left to right, as the terms are formed, so no term exceeds its bound).  Each term is rounded once, to
 * llrint(term / q) (an exact division, nearest even), the terms are added as int64 (below 2^63 by the choice of q) and a box's
 * output is (double)sum * q.  So |sum - exact| <= count q / 2 plus the last bit of the result, for every quantity and box.
 * 2 wmax M, wmax dmax dmax M and wmax smax M must be finite: OISAT_EINVAL after the launches otherwise, the host outputs untouched.
 * 0 <= m <= 1 << 20 (m = 0: zeros), box_deg finite and in (0, 180], a table as above, non-NULL count_out and, where m > 0,
 * non-NULL inputs and box_out; anything else is OISAT_EINVAL and writes nothing.
 * Workspace: 64 B + 12 nbands B + 8 (1 + OISAT_SUPEROB_NSUMS) nbox B on the handle (1 degree boxes: 3.0 MB), grow-only,
 * allocated at the first call that needs it (oisat_dense_reserve does not cover it).
 * oisat_superob_quanta (host only): q_out[6] = q_W, q_Q, q_D, q_V, q_G, q_P by this rule, for tests and callers that bound the
 * error; m outside 0 .. 1 << 20, a negative or NaN maximum, or one of the three products not finite is OISAT_EINVAL. */
#define OISAT_SUPEROB_NSUMS 8              /* rows of sums_out: W, Q, D, V, G, Px, Py, Pz */
int oisat_superob_boxes(double box_deg, int64_t cap, int32_t* n_out, int64_t* offset_out, int64_t* nbands_out, int64_t* nbox_out);
int oisat_superob_quanta(double wmax, double dmax, double smax, int64_t m, double* q_out);
int oisat_superob(oisat_ctx* h, const double* olat, const double* olon, const double* oxyz, const double* d,
                  const double* sigma_b, const double* var, int64_t m, double box_deg, const int32_t* box_n,
                  const int64_t* box_offset, int64_t nbands, int64_t nbox, int32_t* box_out, int64_t* count_out,
                  double* sums_out, int64_t* nused_out);

#ifdef __cplusplus
}
#endif
#endif /* OISAT_H */
