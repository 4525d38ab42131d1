// The dense solver's factor tables: pure host arithmetic, no kernel and no device call, which the *_cpu tests drive without a
// GPU.  The envelope of S in block rows (oisat_envelope*), the factor's own narrower envelope and its far, middle
// and near stretches (oisat_factor_envelope* / _far* / _mid* / _near*, with the measurements behind their cut-offs), and the checks of
// the tables a caller hands back (envelope_table_ok, far_table_ok, mid_table_ok, near_table_ok: dense_internal.h).
#include "dense_internal.h"

using namespace oisat_dense;

namespace {

#include "dense_tile.inc"

#include "dense_solve_dev.inc"                                  // (the correlation functions: lat_window_deg, kCutBits)

}  // namespace

bool oisat_dense::envelope_table_ok(const int32_t* first, int64_t nb) {
    for (int64_t i = 0; i < nb; ++i)
        if (first[i] < 0 || first[i] > (i > 0 ? i - 1 : 0) || (i > 0 && first[i] < first[i - 1])) return false;
    return true;
}

// The fp32 factor's own cut-off.  The factor is only the preconditioner of oisat_gain_solve, which refines against the
// float64 residual of the true S (that residual keeps kCutBits): entries of S far below what an fp32 factorization loses by
// itself (first residual 3e-6 .. 2.4e-5) are work the result does not need.  Chosen by a sweep on MI355X over the headline
// month in three species and the month of test_dense_config3_full_size_properties (profiles/EXPERIMENTS.md, "The factor's
// own cut-off"): 40 .. 24 bits leave the first residual within 0.7 %, the number of solves and the
// last residual (within 6 %) where 52 bits have them on all four months, 20 bits raise the first residual by 6 - 8 %.  Kept:
// the smallest admissible value, 24, plus 4 bits of headroom for a month denser than the benchmark's (the dropped row sums
// of a 1e5-observation month lie ~4 bits above those of a 2e4-observation month).  Headline: 2 520 648 of 4 549 882 K-steps.
constexpr double kFactorCutBits = 28.0;
// The narrow table is used only where it buys time: a step of the factorization's chain costs ~47 us, a 128-deep K-block
// ~15.9 us of one of 512 workgroup slots, so tile work outlasts the chain once a block row holds more than
// 47 x 512 / 15.9 ~ 1 500 K-steps.  Below that (config 2: 228, a 2e4-observation swath month: 251) the launch IS its chain,
// fewer K-steps win nothing, and the factor keeps the 2^-52 table and with it the bits it has always had.
constexpr double kFactorMinKstepsPerRow = 1500.0;

// first | last for the pairs whose correlation can reach 2^-bits (lat_sorted checked by the caller): their latitudes differ
// by at most the angle of that cut-off's chord, great-circle distance >= latitude difference
static void envelope_table(int kind, const double* lat_sorted, int64_t m, double g, double bits, int32_t* env_out) {
    const int64_t nb = cdiv(m, NB);
    const double angle = g > 0.0 ? lat_window_deg(kind, g, bits) : 1e9;
    int64_t k = 0;
    for (int64_t i = 0; i < nb; ++i) {
        const double lo = lat_sorted[i * NB] - angle;           // tile k is outside when lat_max(tile k) < lat_min(tile i) - angle
        while (k < i && lat_sorted[std::min((k + 1) * NB, m) - 1] < lo) ++k;
        env_out[i] = (int32_t)std::min<int64_t>(k, i > 0 ? i - 1 : 0);
    }
    for (int64_t b = 0, j = 0; b < nb; ++b) {                   // last[b] = max{ j : first[j] <= b }
        while (j + 1 < nb && env_out[j + 1] <= b) ++j;
        env_out[nb + b] = (int32_t)j;
    }
}

// K-loop steps of the enveloped factorization: sum over the tiles (i, j) inside the table of j - max(first[i], first[j])
static int64_t envelope_ksteps(const int32_t* first, int64_t nb) {
    int64_t k = 0;
    for (int64_t i = 0; i < nb; ++i)
        for (int64_t j = first[i]; j <= i; ++j) k += j - std::max(first[i], first[j]);
    return k;
}

static bool lat_sorted_ok(const double* lat_sorted, int64_t m) {
    for (int64_t i = 1; i < m; ++i)
        if (!(lat_sorted[i] >= lat_sorted[i - 1])) return false;
    return true;
}

// <n> bits from the environment variable `name` (read at every call, like OISAT_ENVELOPE): lo <= n <= kCutBits into *bits and
// *set = true; unset or empty: *bits stays
static int env_bits(const char* name, double lo, double* bits, bool* set) {
    const int parsed = factor_bits_switch(name, bits);
    *set = parsed != 0;
    ARG_CHECK(parsed >= 0 && (!*set || (*bits >= lo && *bits <= kCutBits)));
    return OISAT_OK;
}

// the default rule (kFactorMinKstepsPerRow): the narrow table `first` pays
static bool narrow_table_pays(const int32_t* first, int64_t nb) {
    return (double)envelope_ksteps(first, nb) > kFactorMinKstepsPerRow * (double)nb;
}

extern "C" int oisat_envelope_corr(int kind, const double* lat_sorted, int64_t m, double g, int32_t* env_out) {
    ARG_CHECK(corr_kind_ok(kind) && lat_sorted && env_out && m > 0 && g >= 0.0);
    ARG_CHECK(lat_sorted_ok(lat_sorted, m));
    envelope_table(kind, lat_sorted, m, g, kCutBits, env_out);  // the same cut-off as the float64 residual and the increment
    return OISAT_OK;
}

extern "C" int oisat_envelope(const double* lat_sorted, int64_t m, double g, int32_t* env_out) {
    return oisat_envelope_corr(OISAT_CORR_GAUSSIAN, lat_sorted, m, g, env_out);
}

// kFactorCutBits, kFactorMinKstepsPerRow and kFactorFarBits below were measured for the Gaussian only.  Gaspari-Cohn reaches
// 2^-28 and 2^-18 at 99.5 % and 97 % of its support radius, so there is no narrower table worth having: its factor's envelope
// IS the support envelope (oisat_envelope_corr's, which drops exact zeros only), with no chain-bound fallback to decide, and
// its far table is empty (far = first).  SOAR, and any model that is not the Gaussian, takes the same rule -- the 2^-52 table,
// far = first, mid = far -- because nothing has been measured for it.  The environment variables still force their rules,
// through cut_chord.
extern "C" int oisat_factor_envelope_corr(int kind, const double* lat_sorted, int64_t m, double g, int32_t* env_out) {
    ARG_CHECK(corr_kind_ok(kind) && lat_sorted && env_out && m > 0 && g >= 0.0);
    ARG_CHECK(lat_sorted_ok(lat_sorted, m));
    double bits = kFactorCutBits;
    bool forced = false;
    if (int rc = env_bits("OISAT_FACTOR_CUT_BITS", 1.0, &bits, &forced)) return rc;
    if (kind != OISAT_CORR_GAUSSIAN && !forced) bits = kCutBits;
    envelope_table(kind, lat_sorted, m, g, bits, env_out);
    if (kind == OISAT_CORR_GAUSSIAN && !forced && !narrow_table_pays(env_out, cdiv(m, NB)))
        envelope_table(kind, lat_sorted, m, g, kCutBits, env_out);     // chain-bound: nothing to win, keep the float64 sums' table
    return OISAT_OK;
}

extern "C" int oisat_factor_envelope(const double* lat_sorted, int64_t m, double g, int32_t* env_out) {
    return oisat_factor_envelope_corr(OISAT_CORR_GAUSSIAN, lat_sorted, m, g, env_out);
}

// The far stretch of the factor's K-loops.  Left of the 2^-kFactorCutBits table every entry of S is dropped; just inside it, in
// the block columns first[i] <= k < far[i], every correlation between an observation of block row i and one of block column k
// is still below 2^-kFactorFarBits, and the products L(i,k) L(j,k)^T of those K-blocks add terms bounded by such entries.  The
// factor is a preconditioner (kFactorCutBits above): rounding BOTH operands of those products to bf16 -- relative error 2^-8
// of a term that small -- is of the order of what the cut-off drops already, and the bf16 matrix pipe issues them at 1/16 of
// the fp32 pipe's cycles (dense_dag.inc: dag_seg_bf16).  On by default only where the narrow table is: tile-work-bound
// systems, no forced OISAT_FACTOR_CUT_BITS.  OISAT_FACTOR_FAR_BITS=<n> (read at every call): 0 = off; 1 .. 52 forces 2^-n
// at every enveloped size (also under a forced cut-off; a value at or above the table's own cut-off leaves nothing far).
// The value is a measurement, by the protocol of kFactorCutBits (profiles/EXPERIMENTS.md, "The far stretch on the bf16 pipe"): on
// the same four months 24 .. 14 bits leave the first residual within 1.0 % of the run without a stretch, the number of solves
// and the last residual (within 4 %) where they were; 12 bits raise the first residual by 6 - 14 %.  Kept: the smallest
// admissible value, 14, plus 4 bits of headroom for a denser month.  Headline: 872 522 of 2 519 868 K-blocks are far (0.346),
// potrf_dag 84.0 -> 67.2 ms, the step 100.6 -> 83.8 ms.
constexpr double kFactorFarBits = 18.0;

// A stretch of the factor's K-loops as a table: out[i] = the table of cut-off 2^-bits clamped into [lower[i], i] -- lower: the table
// below it, `first` for the far stretch, `far` for the middle one -- or lower[i] where the stretch is off.  bits: `def` under the
// default rule -- on exactly where the narrow table is: Gaussian, tile-work-bound, no forced OISAT_FACTOR_CUT_BITS --, or the <n>
// of the variable `var`: 0 = off, 1 .. 52 forces 2^-n at every enveloped size.  Never on under OISAT_ENVELOPE=0.
// all_ok (the near stretch): the variable may also say `all`, and `def` may be kFactorNearAll -- the whole rest of the row, out[i] = i,
// no cut-off at all; a `def` of 0 is a stretch that is off unless forced.
constexpr double kFactorNearAll = -1.0;
static int stretch_table(const char* var, double def, int kind, const double* lat_sorted, int64_t m, double g, const int32_t* lower, int32_t* out,
                         bool all_ok = false) {
    const int64_t nb = cdiv(m, NB);
    double bits = def;
    bool on = false, forced = false;
    if (all_ok && factor_near_all()) {
        bits = kFactorNearAll;
        forced = true;
    } else if (int rc = env_bits(var, 0.0, &bits, &forced)) {
        return rc;
    }
    std::vector<int32_t> t(2 * (size_t)nb);
    if (forced) {
        on = bits >= 1.0 || bits == kFactorNearAll;
        ARG_CHECK(on || bits == 0.0);
    } else if (def != 0.0) {
        if (!factor_cut_bits_set() && kind == OISAT_CORR_GAUSSIAN) {        // the default rule's own choice: the narrow table, or not
            envelope_table(kind, lat_sorted, m, g, kFactorCutBits, t.data());
            on = narrow_table_pays(t.data(), nb);
        }
    }
    on = on && !oisat_envelope_off();
    if (on && bits != kFactorNearAll) envelope_table(kind, lat_sorted, m, g, bits, t.data());
    if (on && bits == kFactorNearAll)
        for (int64_t i = 0; i < nb; ++i) t[i] = (int32_t)i;
    for (int64_t i = 0; i < nb; ++i) out[i] = on ? std::min<int32_t>(std::max(t[i], lower[i]), (int32_t)i) : lower[i];
    return OISAT_OK;
}

extern "C" int oisat_factor_far_corr(int kind, const double* lat_sorted, int64_t m, double g, const int32_t* first, int32_t* far_out) {
    ARG_CHECK(corr_kind_ok(kind) && lat_sorted && first && far_out && m > 0 && g >= 0.0);
    ARG_CHECK(lat_sorted_ok(lat_sorted, m));
    ARG_CHECK(envelope_table_ok(first, cdiv(m, NB)));
    return stretch_table("OISAT_FACTOR_FAR_BITS", kFactorFarBits, kind, lat_sorted, m, g, first, far_out);
}

extern "C" int oisat_factor_far(const double* lat_sorted, int64_t m, double g, const int32_t* first, int32_t* far_out) {
    return oisat_factor_far_corr(OISAT_CORR_GAUSSIAN, lat_sorted, m, g, first, far_out);
}

extern "C" int oisat_set_factor_far(oisat_ctx* h, const int32_t* far, int64_t nb) {
    ARG_CHECK(h != nullptr && nb >= 0 && (far != nullptr || nb == 0));
    h->factor_far.assign(far, far + nb);
    return OISAT_OK;
}

// the table the caller set for this factorization (empty: none) against its envelope
bool oisat_dense::far_table_ok(const std::vector<int32_t>& far, const int32_t* first, int64_t nb) {
    if (far.empty()) return true;
    if ((int64_t)far.size() != nb) return false;
    for (int64_t i = 0; i < nb; ++i)
        if (far[i] < first[i] || far[i] > i) return false;
    return true;
}

// The middle stretch of the factor's K-loops: the block columns far[i] <= k < mid[i] of block row i, between the far stretch
// and the fp32 rest.  Every correlation between an observation of block row i and one of those block columns is below
// 2^-kFactorMidBits; the products of those K-blocks run on the bf16 pipe as SPLIT products (dense_dag.inc: dag_seg_bf16x2,
// hi hi^T + hi lo^T + lo hi^T, relative error ~2^-16 instead of the far stretch's 2^-8), 3/16 of the fp32 pipe's MFMA cycles.
// The argument is the far stretch's, eight bits further in: an error of 2^-16 of a term bounded by 2^-f.  On by default exactly
// where the far stretch is (Gaussian, tile-work-bound, no forced OISAT_FACTOR_CUT_BITS, not OISAT_ENVELOPE=0).
// OISAT_FACTOR_MID_BITS=<n> (read at every call): 0 = off (mid = far); 1 .. 52 forces 2^-n at every enveloped size; an n at or
// above the far cut-off in force leaves nothing in the middle (the table is clamped to far[i] <= mid[i] <= i), and with the far
// stretch off the middle one starts at first[i].
// The value is a measurement, by the protocol of kFactorFarBits (profiles/EXPERIMENTS.md, "The middle stretch as split bf16
// products"; profiles/mid_band_sweep.json): on the same four months, far stretch at 2^-18, OISAT_FACTOR_MID_BITS = 16 .. 6
// leave the first residual within +1.3 % / -0.6 % of the run without a middle stretch, one correction converges, the last
// residual within 8 %; 4 bits, the smallest value swept, are still admissible by the rule (first residual <= 1.05 x: it is
// 1.5 - 3.6 % up, the last residual 2 - 6 %) but the rise has begun -- the host emulation puts the break between 6 and 4.
// Kept: the smallest admissible value, 4, plus 4 bits of headroom for a denser month.  Headline: 892 351 of 2 519 868 K-blocks
// are middle (0.354) next to 872 522 far ones (0.346); the step falls by 2.9 ms per 0.1 of share, against 4.7 for the far
// stretch: a middle K-block costs about 0.6 of an fp32 one.  potrf_dag 66.9 -> 56.5 ms, the step 84.6 - 84.8 -> 74.4 - 74.6 ms.
constexpr double kFactorMidBits = 8.0;

extern "C" int oisat_factor_mid_corr(int kind, const double* lat_sorted, int64_t m, double g, const int32_t* first, const int32_t* far,
                                     int32_t* mid_out) {
    ARG_CHECK(corr_kind_ok(kind) && lat_sorted && first && far && mid_out && m > 0 && g >= 0.0);
    ARG_CHECK(lat_sorted_ok(lat_sorted, m));
    const int64_t nb = cdiv(m, NB);
    ARG_CHECK(envelope_table_ok(first, nb));
    for (int64_t i = 0; i < nb; ++i) ARG_CHECK(far[i] >= first[i] && far[i] <= i);
    return stretch_table("OISAT_FACTOR_MID_BITS", kFactorMidBits, kind, lat_sorted, m, g, far, mid_out);
}

extern "C" int oisat_factor_mid(const double* lat_sorted, int64_t m, double g, const int32_t* first, const int32_t* far, int32_t* mid_out) {
    return oisat_factor_mid_corr(OISAT_CORR_GAUSSIAN, lat_sorted, m, g, first, far, mid_out);
}

extern "C" int oisat_set_factor_mid(oisat_ctx* h, const int32_t* mid, int64_t nb) {
    ARG_CHECK(h != nullptr && nb >= 0 && (mid != nullptr || nb == 0));
    h->factor_mid.assign(mid, mid + nb);
    return OISAT_OK;
}

// the middle table the caller set for this factorization (empty: none) against its envelope and its far table (empty: first)
bool oisat_dense::mid_table_ok(const std::vector<int32_t>& mid, const std::vector<int32_t>& far, const int32_t* first, int64_t nb) {
    if (mid.empty()) return true;
    if ((int64_t)mid.size() != nb || !far_table_ok(far, first, nb)) return false;
    for (int64_t i = 0; i < nb; ++i)
        if (mid[i] < (far.empty() ? first[i] : far[i]) || mid[i] > i) return false;
    return true;
}

// The near stretch of the factor's K-loops: the block columns mid[i] <= k < near[i] of block row i, between the middle stretch
// and what is left for the fp32 pipe.  Their products run on the bf16 pipe as THREE-WAY split products (dense_dag.inc:
// dag_seg_bf16x3: eight bf16 products per fp32 one, only lo lo^T dropped: <= 2^-32 of a term), 1/2 of the fp32 pipe's MFMA cycles.
// The split is exact and the products are accurate far beyond fp32's rounding, and still the stretch is NOT free next to the
// diagonal, where L's entries are large: the sum of eight partial products per k-chunk, each rounded into the fp32 accumulator, is
// not the fp32 pipe's sum of exact products.  So the cut-off is a measurement like the other two.  On by default exactly where they
// are (Gaussian, tile-work-bound, no forced OISAT_FACTOR_CUT_BITS, not OISAT_ENVELOPE=0).  OISAT_FACTOR_NEAR_BITS (read at every
// call): 0 = off (near = mid, the launch of the code before the stretch, bit for bit); 1 .. 52 forces the table of 2^-n at every
// enveloped size (clamped to mid[i] <= near[i] <= i); `all` = the whole rest of every row, near[i] = i (kFactorNearAll).  The
// chain's own products stay fp32 whatever the table says.
// The value, by the protocol of kFactorMidBits (profiles/EXPERIMENTS.md, "The near stretch as three-way split bf16 products";
// profiles/near_band_sweep.json): on the same four months, far 2^-18 and middle 2^-8, OISAT_FACTOR_NEAR_BITS = 2 leaves the first
// residual within +1.7 % of the run without the stretch; 1 raises it by 2.7 - 4.4 % (admissible: <= 1.05 x, one correction, last
// residual <= 1.12 x); `all` raises it by 11.5 - 12.4 % on all four and is NOT admissible (with six products: 10 - 13 %, the
// same).  Kept: the widest admissible value, 1.  Headline: 650 997 of 2 519 868 K-blocks are near (0.258), 0.041 stay on the fp32
// pipe; the step falls by 1.1 - 1.3 ms.
constexpr double kFactorNearBits = 1.0;

extern "C" int oisat_factor_near_corr(int kind, const double* lat_sorted, int64_t m, double g, const int32_t* first, const int32_t* mid,
                                      int32_t* near_out) {
    ARG_CHECK(corr_kind_ok(kind) && lat_sorted && first && mid && near_out && m > 0 && g >= 0.0);
    ARG_CHECK(lat_sorted_ok(lat_sorted, m));
    const int64_t nb = cdiv(m, NB);
    ARG_CHECK(envelope_table_ok(first, nb));
    for (int64_t i = 0; i < nb; ++i) ARG_CHECK(mid[i] >= first[i] && mid[i] <= i);
    return stretch_table("OISAT_FACTOR_NEAR_BITS", kFactorNearBits, kind, lat_sorted, m, g, mid, near_out, true);
}

extern "C" int oisat_factor_near(const double* lat_sorted, int64_t m, double g, const int32_t* first, const int32_t* mid, int32_t* near_out) {
    return oisat_factor_near_corr(OISAT_CORR_GAUSSIAN, lat_sorted, m, g, first, mid, near_out);
}

extern "C" int oisat_set_factor_near(oisat_ctx* h, const int32_t* near, int64_t nb) {
    ARG_CHECK(h != nullptr && nb >= 0 && (near != nullptr || nb == 0));
    h->factor_near.assign(near, near + nb);
    return OISAT_OK;
}

// the near table the caller set for this factorization (empty: none) against its envelope and the tables below it (empty: the one below)
bool oisat_dense::near_table_ok(const std::vector<int32_t>& near, const std::vector<int32_t>& mid, const std::vector<int32_t>& far,
                                const int32_t* first, int64_t nb) {
    if (near.empty()) return true;
    if ((int64_t)near.size() != nb || !mid_table_ok(mid, far, first, nb)) return false;
    for (int64_t i = 0; i < nb; ++i)
        if (near[i] < (!mid.empty() ? mid[i] : !far.empty() ? far[i] : first[i]) || near[i] > i) return false;
    return true;
}
