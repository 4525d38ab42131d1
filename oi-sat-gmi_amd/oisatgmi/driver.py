"""The ``oisatgmi`` facade -- hot-path methods on the MI355X.

Drop-in for the methods of ``oisatgmi/driver.py`` that lie on the optimal-interpolation path:
``average`` (:53-63), ``bias_correct`` (:65-106) and ``oi`` (:108-114), the two vertical operators
feeding them -- ``recal_amf`` (:35-38), ``cal_pwv`` (:42-44) and ``conv_ak`` (:46-51) -- and the output stage ``write_to_nc``
(:156-227; same variables, the scaling-factor rule evaluated on the device), with the same attribute
names set on ``self``; ``savedaily`` (:135-155) is plain file writing and is kept as is.  The remaining methods
of the reference's class (``read_data``, ``reporting``) are file formats and plotting outside this path: they raise ``NotImplementedError`` here -- see INTEGRATION.md
for binding the HIP path into the reference's own class instead.
"""
from __future__ import annotations

import numpy as np

import os

from . import _hip
from .averaging import averaging
from .optimal_interpolation import OI

#: (sensor, gas) -> (offset, slope) of the validated linear bias corrections, driver.py:68-100
BIAS_CORRECTIONS = {
    ("TROPOMI", "NO2"): (0.32, 0.66),
    ("TROPOMI", "HCHO"): (0.90, 0.59),
    ("OMI", "NO2"): (0.32, 0.63),
    ("OMI", "HCHO"): (0.821, 0.79),
}

#: DU <-> 1e15 molec/cm2 factor applied to the model O3 column, driver.py:62-63
O3_DIVISOR = 2.69e16 * 1e-15


class oisatgmi(object):

    def __init__(self) -> None:
        pass

    # ---- hot path ---------------------------------------------------------------------------
    def average(self, startdate: str, enddate: str, gasname=None):
        """Monthly means of what the reader holds between the two ``'YYYY-mm-dd'`` dates (driver.py:53-70); ``gasname='O3'``
        additionally converts the model column to Dobson units."""
        (self.sat_averaged_vcd, self.sat_averaged_error, self.ctm_averaged_vcd, self.aux1, self.aux2,
         self.avg_time) = averaging(startdate, enddate, self.reader_obj)
        self._granule_grid = None
        if gasname == 'O3':
            self.ctm_averaged_vcd = self.ctm_averaged_vcd / O3_DIVISOR

    def average_granules(self, startdate: str, enddate: str, granules, interpolator_type, grid_size, flag_thresh=0.75,
                         gasname=None, keep_daily=False):
        """``average`` straight from a month of RAW granules (``oisatgmi.month.month_average``): regrid, AMF recalculation
        (``satellite_amf``) or averaging-kernel convolution (``satellite_opt``; the sensor, MOPITT or GOSAT, comes from the
        records) against ``reader_obj.ctm_data`` and averaging without the regridded granules ever leaving the device.
        Sets the attributes ``average`` sets, bit for bit those of regridding with ``interpolator_many``, ``recal_amf`` or
        ``conv_ak`` and ``average``, so ``oi('GOSAT')`` reads aux1 / aux2 as it does after ``average``.
        ``keep_daily=True`` also fills ``reader_obj.sat_data`` with slim per-granule records for ``savedaily``."""
        from .month import _month_average
        ctm_data = self.reader_obj.ctm_data
        coord = {"Latitude": ctm_data[0].latitude, "Longitude": ctm_data[0].longitude}      # reader.py:1519-1520
        res, daily, self._granule_grid = _month_average(startdate, enddate, granules, ctm_data, coord, interpolator_type,
                                                        grid_size, flag_thresh, None, keep_daily)
        if keep_daily:
            self.reader_obj.sat_data = daily
        (self.sat_averaged_vcd, self.sat_averaged_error, self.ctm_averaged_vcd, self.aux1, self.aux2, self.avg_time) = res
        if gasname == 'O3':
            self.ctm_averaged_vcd = self.ctm_averaged_vcd / O3_DIVISOR

    def _first_granule_grid(self):
        """(lon, lat) of the averaged grid: the first granule record's, or the grid ``average_granules`` averaged onto."""
        grid = getattr(self, "_granule_grid", None)
        if grid is not None:
            return grid
        first = next(g for g in self.reader_obj.sat_data if g is not None)
        return first.longitude_center, first.latitude_center

    def bias_correct(self, sat_type, gasname):
        # apply bias correction based on several validation studies
        corr = BIAS_CORRECTIONS.get((sat_type, gasname))
        if corr is None:
            print("NOT applying the bias correction for satellite VCDs")
            return
        print("applying the bias correction for " + str(sat_type) + " " + str(gasname))
        offset, slope = corr
        self.sat_averaged_vcd = (self.sat_averaged_vcd - offset) / slope

    # ---- analysis mode (extension; the signature of oi() is the reference's) -----------------------------
    #   mode        attribute `oi_mode`        | env OISAT_OI_MODE        diag (default) | dense | tiled
    #   L           attribute `corr_length_km` | env OISAT_CORR_LENGTH_KM km, default 300, or `auto`: fitted to the covariogram of
    #               the month's own innovations (dense.estimate_corr_length; oi_info["corr_fit"]; 300 if no fit is found)  (dense, tiled)
    #   model       attribute `oi_correlation` | env OISAT_CORRELATION    gaussian (default) | gaspari_cohn | soar  (dense, tiled)
    #   tile size   attribute `tile_deg`       | env OISAT_TILE_DEG       degrees, default 30       (tiled; halo = 3 L,
    #               gaspari_cohn: its support 3.65 L, soar: 6.52 L)
    #   unobserved  attribute `oi_unobserved`  | env OISAT_UNOBSERVED     nan (default) | xa        (dense, tiled)
    #   grid        attributes `grid_lat`, `grid_lon` (ny, nx), else the first granule's latitude_center/longitude_center
    #   knee        attribute `oi_reg_index`: force the index into the 99-scaling sweep (all modes)
    #   error/AK    attribute `oi_want_error`  | env OISAT_OI_ERROR       1 (default) | 0: error_OI / ak_OI left NaN -- the
    #               posterior error costs n m^2 flop, 1e16 for a global 720x1440 / 1e5-observation analysis (dense, tiled)
    #               mc | mc:<K> (dense only): the randomized estimate of both from K probes (default 256, a multiple of 128)
    #               through the factor the analysis leaves behind, with its own standard errors in oi_info["err_se"] /
    #               ["ak_obs_se"] (dense.DenseAnalysis.posterior_error_mc); tiled: ValueError -- the
    #               tiles' exact error is affordable
    #   QC          attribute `oi_qc`          | env OISAT_OI_QC          off (default) | buddy | buddy:<k_buddy>  (dense, tiled;
    #               diag ignores it): background check and buddy check of the innovations ahead of the analysis
    #               (dense.qc_innovations) at the analysis' L -- under `auto` at the length fitted to all
    #               observations (oi_info["qc"]["corr_fit_before"]), and the analysis' length is then refitted to the kept ones;
    #               a rejected cell is analysed as unobserved; oi_info["qc"], oi_info["qc_rejected"]
    #   superob     attribute `oi_superob`     | env OISAT_OI_SUPEROB     off (default) | <deg> | auto | auto:<max_obs>  (dense only;
    #               tiled: ValueError; diag ignores it): the KEPT observations of one box of <deg> degrees (a roughly equal-area
    #               grid) are merged into one superobservation ahead of the analysis, whose system then has one row per
    #               non-empty box (dense.superob); auto: nothing while the observations number at most
    #               max_obs (default 100 000), else the smallest box of 0.5, 0.75, 1, 1.5, 2, 3, 4, 6 degrees that leaves at
    #               most max_obs; a box wider than L / 2 is reported in one line; oi_info["superob"]
    #   regions     attribute `oi_regions`     | env OISAT_OI_REGIONS     off (default) | an (ny, nx) integer label map, or the
    #               path of a .npy file that holds one (the variable: a path)  (dense only; diag, tiled: ValueError): values <= 0
    #               are no region, at most 64 regions.  The analysis then reports each region's area-weighted mean before and
    #               after and the EXACT error of that mean, error correlations between cells included, with the covariances
    #               between the regions (dense.DenseAnalysis.functional_covariance); region_OI,
    #               oi_info["regions"]
    #   scale       attribute `oi_scale`       | env OISAT_OI_SCALE       knee (default) | ml | ml:both  (dense only; diag, tiled:
    #               ValueError): knee = the regularisation factor of the reference's knee sweep, as before.  ml: that factor is
    #               the starting point, and the amplitude of B is then estimated by maximum likelihood of the month's innovations
    #               under S = s H B H^T + R itself (dense.DenseAnalysis.fit_error_scales); ml:both also
    #               estimates a common inflation of the observation errors (the masks of error_OI / ak_OI keep So as given).
    #               The knee still feeds the `auto` length and the QC, which come first.  oi_info["scale"] = knee x scale_b,
    #               oi_info["scale_knee"], oi_info["scale_fit"], oi_info["likelihood"]
    #   ensemble    attribute `oi_ensemble`    | env OISAT_OI_ENSEMBLE    off (default) | <K> | <K>:<F>  (dense only; diag, tiled:
    #               ValueError): K draws (a positive multiple of 32) from the analysis' own error distribution N(0, A) by
    #               Matheron's rule, each from F random features (default 256), through the factor the analysis leaves behind
    #               (dense.DenseAnalysis.posterior_ensemble; gaussian and soar); oi_info["ensemble"]:
    #               deviations (K, ny, nx), NaN where the background is, and the err / err_se they imply.  error_OI / ak_OI
    #               and OISAT_OI_ERROR are untouched
    #   drift       attribute `oi_drift`       | env OISAT_OI_DRIFT       off (default) | <degree> 0..3  (dense only; diag, tiled:
    #               ValueError): a large-scale mean of the innovations -- the (degree + 1)^2 real harmonics up to that degree,
    #               e.g. a model that runs low over a hemisphere -- is estimated together with the analysis (universal kriging,
    #               dense.DenseAnalysis.run(drift=...)) instead of being spread as a correlated anomaly;
    #               the four attributes include it (error_OI with the variance the unknown drift adds), oi_info["drift"]: beta,
    #               beta_se, cond, chi2, var.  Not combined with oi_scale = ml, oi_ensemble or oi_regions yet (ValueError)
    def _oi_setting(self, attr, env, default, cast=str):
        v = getattr(self, attr, None)
        if v is None:
            v = os.environ.get(env)
        return cast(default if v in (None, "") else v)

    @staticmethod
    def _corr_length(v):
        """A length in km, or ``"auto"`` (any case): estimate it from the innovations.  Anything else is a ``ValueError``."""
        if isinstance(v, str) and v.strip().lower() == "auto":
            return "auto"
        return float(v)

    @staticmethod
    def _error_setting(v):
        """``OISAT_OI_ERROR`` / ``oi_want_error`` -> ``(want_error, nprobe)``: ``(False, 0)`` for 0 / false / no / off,
        ``("mc", K)`` for ``mc`` / ``mc:<K>`` (K a positive multiple of 128; anything else behind ``mc`` is a ``ValueError``),
        ``(True, 0)`` for every other value, as before."""
        v = str(v).strip().lower()
        if v in ("0", "false", "no", "off"):
            return False, 0
        if not v.startswith("mc"):
            return True, 0
        if v == "mc":
            return "mc", 256
        try:
            if v[2] != ":":
                raise ValueError
            K = int(v[3:])
        except ValueError:
            raise ValueError(f"OISAT_OI_ERROR / oi_want_error: expected mc or mc:<probes>, not {v!r}") from None
        if K < 128 or K % 128:
            raise ValueError(f"OISAT_OI_ERROR / oi_want_error: the number of probes must be a positive multiple of 128, not {K}")
        return "mc", K

    @staticmethod
    def _qc_setting(v):
        """``OISAT_OI_QC`` / ``oi_qc`` -> ``None`` for ``off``, ``{"k_buddy": k}`` for ``buddy`` (k = 3) / ``buddy:<k_buddy>`` (a
        positive finite float); anything else is a ``ValueError``."""
        v = str(v).strip().lower()
        if v == "off":
            return None
        if v == "buddy":
            return {"k_buddy": 3.0}
        try:
            if not v.startswith("buddy:"):
                raise ValueError
            k = float(v[6:])
            if not (0.0 < k < float("inf")):
                raise ValueError
        except ValueError:
            raise ValueError(f"OISAT_OI_QC / oi_qc: expected off, buddy or buddy:<k_buddy> (a positive number), not {v!r}") from None
        return {"k_buddy": k}

    @staticmethod
    def _scale_setting(v):
        """``OISAT_OI_SCALE`` / ``oi_scale`` -> ``None`` for ``knee``, ``"background"`` for ``ml``, ``"both"`` for ``ml:both`` (the
        ``fit_scale`` of ``dense.OI_dense``); anything else is a ``ValueError``."""
        modes = {"knee": None, "ml": "background", "ml:both": "both"}
        try:
            return modes[str(v).strip().lower()]
        except KeyError:
            raise ValueError(f"OISAT_OI_SCALE / oi_scale: expected knee, ml or ml:both, not {v!r}") from None

    @staticmethod
    def _ensemble_setting(v):
        """``OISAT_OI_ENSEMBLE`` / ``oi_ensemble`` -> ``None`` for ``off``, ``(K, F)`` for ``<K>`` (F = 256) / ``<K>:<F>`` (K a
        positive multiple of 32, F >= 1); anything else is a ``ValueError``."""
        from . import dense
        t = str(v).strip().lower()
        if t == "off":
            return None
        try:
            parts = t.split(":")
            if len(parts) > 2:
                raise ValueError
            return dense._ensemble_sizes(int(parts[0]), int(parts[1]) if len(parts) == 2 else 256)
        except ValueError:
            raise ValueError(f"OISAT_OI_ENSEMBLE / oi_ensemble: expected off, <members> or <members>:<features> (members a positive "
                             f"multiple of 32, features at least 1), not {v!r}") from None

    @staticmethod
    def _drift_setting(v):
        """``OISAT_OI_DRIFT`` / ``oi_drift`` -> ``None`` for ``off``, the degree 0..3 for ``<degree>``; anything else is a
        ``ValueError``."""
        from . import dense
        t = str(v).strip().lower()
        if t == "off":
            return None
        try:
            return dense.drift_degree(int(t))
        except ValueError:
            raise ValueError(f"OISAT_OI_DRIFT / oi_drift: expected off or a degree 0..{dense.DRIFT_MAX_DEGREE}, not {v!r}") from None

    @staticmethod
    def _superob_setting(v):
        """``OISAT_OI_SUPEROB`` / ``oi_superob`` -> ``None`` for ``off``, the box size in degrees (a float in (0, 180]) for
        ``<deg>``, ``"auto:<max_obs>"`` for ``auto`` (max_obs = 100 000) / ``auto:<max_obs>`` (a positive integer); anything else
        is a ``ValueError``."""
        from . import dense
        try:
            box, max_obs = dense.superob_setting(v)
        except ValueError:
            raise ValueError(f"OISAT_OI_SUPEROB / oi_superob: expected off, <degrees> in (0, 180], auto or auto:<max_obs> "
                             f"(a positive integer), not {v!r}") from None
        return f"auto:{max_obs}" if box == "auto" else box

    def _regions_setting(self):
        """``oi_regions`` (an array or a path) / ``OISAT_OI_REGIONS`` (a path) -> the label map, or ``None`` when neither is set."""
        v = getattr(self, "oi_regions", None)
        if v is None:
            v = os.environ.get("OISAT_OI_REGIONS") or None
        if v is None:
            return None
        if isinstance(v, (str, os.PathLike)):
            try:
                v = np.load(os.fspath(v), allow_pickle=False)
            except (OSError, ValueError) as e:
                raise ValueError(f"OISAT_OI_REGIONS / oi_regions: cannot read a .npy label map from {v!r}: {e}") from None
        return np.asarray(v)

    def _oi_grid(self):
        lat, lon = getattr(self, "grid_lat", None), getattr(self, "grid_lon", None)
        if lat is None or lon is None:
            lon, lat = self._first_granule_grid()
        return np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)

    def oi(self, sensor: str, error_ctm=50.0):
        """driver.py:108-114.  Default (``diag``): the reference's element-wise analysis.  ``dense`` / ``tiled``: the
        Gaussian-B generalisation x_a = x_b + B H^T (H B H^T + R)^-1 (y - H x_b) with B = s D^1/2 C D^1/2 -- global, or
        localised to tiles with a 3 L halo; D = diag(Sa) and R = diag(So) are the reference's variances, s is the
        regularisation factor picked by the reference's own knee sweep over the element-wise curve
        (optimal_interpolation.py:15-41), and L -> 0 reproduces the ``diag`` attributes at observed cells.  The same
        four attributes are filled.  Unobserved cells: ``nan`` (default) keeps the reference's convention -- NaN in all
        four fields, optimal_interpolation.py:49-50 with Y = NaN; ``xa`` keeps what the dense analysis really says there:
        background + spread increment, posterior error, averaging kernel 0."""
        if sensor != 'GOSAT':
            xa, y = self.ctm_averaged_vcd, self.sat_averaged_vcd
        else:
            xa, y = self.aux2, self.aux1
        Sa, So = (xa * error_ctm / 100.0) ** 2, self.sat_averaged_error ** 2
        mode = self._oi_setting("oi_mode", "OISAT_OI_MODE", "diag").lower()
        reg_index = getattr(self, "oi_reg_index", None)
        regions = self._regions_setting()
        if regions is not None and mode in ("diag", "tiled"):
            raise ValueError("OISAT_OI_REGIONS / oi_regions belongs to the dense mode; the error of a regional mean needs the error "
                             "correlations between cells, and regions cross tiles (off)")
        fit_scale = self._oi_setting("oi_scale", "OISAT_OI_SCALE", "knee", self._scale_setting)
        if fit_scale is not None and mode in ("diag", "tiled"):
            raise ValueError("OISAT_OI_SCALE / oi_scale = ml belongs to the dense mode; the tiles share the observations of their "
                             "halos, so their likelihoods do not add (knee)")
        ensemble = self._oi_setting("oi_ensemble", "OISAT_OI_ENSEMBLE", "off", self._ensemble_setting)
        if ensemble is not None and mode in ("diag", "tiled"):
            raise ValueError("OISAT_OI_ENSEMBLE / oi_ensemble belongs to the dense mode; the members are drawn through the one factor "
                             "of the whole system, and a tile has none of its neighbours' (off)")
        drift = self._oi_setting("oi_drift", "OISAT_OI_DRIFT", "off", self._drift_setting)
        if drift is not None and mode in ("diag", "tiled"):
            raise ValueError("OISAT_OI_DRIFT / oi_drift belongs to the dense mode; the drift is one set of coefficients for the whole "
                             "system, and a tile sees a part of it (off)")
        if drift is not None:
            for name, v in (("OISAT_OI_SCALE / oi_scale = ml", fit_scale), ("OISAT_OI_ENSEMBLE / oi_ensemble", ensemble),
                            ("OISAT_OI_REGIONS / oi_regions", regions)):
                if v is not None:
                    raise ValueError(f"OISAT_OI_DRIFT / oi_drift cannot be combined with {name} yet (off)")
        if mode == "diag":
            self.ctm_averaged_vcd_corrected, self.ak_OI, self.increment_OI, self.error_OI = OI(
                xa, y, Sa, So, regularization_on=True, reg_index=reg_index)
            return
        if mode not in ("dense", "tiled"):
            raise ValueError(f"OISAT_OI_MODE / oi_mode must be diag, dense or tiled, not {mode!r}")
        L = self._oi_setting("corr_length_km", "OISAT_CORR_LENGTH_KM", 300.0, self._corr_length)
        corr = self._oi_setting("oi_correlation", "OISAT_CORRELATION", "gaussian").lower()
        if corr not in ("gaussian", "gaspari_cohn", "soar"):
            raise ValueError(f"OISAT_CORRELATION / oi_correlation must be gaussian, gaspari_cohn or soar, not {corr!r}")
        unobserved = self._oi_setting("oi_unobserved", "OISAT_UNOBSERVED", "nan").lower()
        if unobserved not in ("nan", "xa"):
            raise ValueError(f"OISAT_UNOBSERVED / oi_unobserved must be nan or xa, not {unobserved!r}")
        want_error, nprobe = self._oi_setting("oi_want_error", "OISAT_OI_ERROR", "1", self._error_setting)
        if want_error == "mc" and mode == "tiled":
            raise ValueError("OISAT_OI_ERROR / oi_want_error = mc belongs to the dense mode; a tiled analysis has the exact error (1)")
        qc = self._oi_setting("oi_qc", "OISAT_OI_QC", "off", self._qc_setting)
        superob = self._oi_setting("oi_superob", "OISAT_OI_SUPEROB", "off", self._superob_setting)
        if superob is not None and mode == "tiled":
            raise ValueError("OISAT_OI_SUPEROB / oi_superob belongs to the dense mode; the tiles take observation values, not "
                             "innovations (off)")
        lat, lon = self._oi_grid()
        xa, y = np.asarray(xa), np.asarray(y)
        if lat.shape != xa.shape[:2] or lon.shape != xa.shape[:2]:
            raise ValueError(f"oi(): the grid is {lat.shape} but the averaged fields are {xa.shape}; set grid_lat / grid_lon "
                             f"(ny, nx) to the model grid the fields live on")
        print('Optimal interpolation begins...')
        y[y < 0] = 0.0                                           # in place, optimal_interpolation.py:14
        tile = self._oi_setting("tile_deg", "OISAT_TILE_DEG", 30.0, float)
        # averaging() hands back (ny, nx) for the one-month windows run/job.py:77-82 passes and (ny, nx, months[, years])
        # for longer ones (averaging.py:53-58,:110-114: squeezed 4-D buffers).  The element-wise OI does not care; a
        # spatial analysis is one analysis per (month, year) slice.
        outs = [np.full(xa.shape, np.nan) for _ in range(4)]
        infos = []
        for tail in np.ndindex(*xa.shape[2:]):
            sl = (slice(None), slice(None)) + tail
            res, info = self._oi_spatial(mode, xa[sl], y[sl], np.asarray(Sa)[sl], np.asarray(So)[sl], lat, lon, L, tile,
                                         unobserved, reg_index, want_error, corr=corr, nprobe=nprobe, qc=qc,
                                         superob=superob, regions=regions, fit_scale=fit_scale, ensemble=ensemble, drift=drift)
            for o, r in zip(outs, res):
                o[sl] = r
            infos.append(info)
        self.ctm_averaged_vcd_corrected, self.ak_OI, self.increment_OI, self.error_OI = outs
        self.oi_info = dict(infos[0]) if len(infos) == 1 else {**infos[0], "slices": infos}
        if regions is not None:                                  # (one dict per (month, year) slice when there are several)
            self.region_OI = infos[0]["regions"] if len(infos) == 1 else [i["regions"] for i in infos]

    @staticmethod
    def _oi_spatial(mode, xa, y, Sa, So, lat, lon, L, tile, unobserved, reg_index, want_error, corr="gaussian", nprobe=256,
                    qc=None, superob=None, regions=None, fit_scale=None, ensemble=None, drift=None):
        """One (ny, nx) Gaussian-B analysis -> ((Xb, AK, increment, error), info) in the reference's attribute order.  ``qc``
        (``_qc_setting``): not None = the innovations are checked first and the rejected cells analysed as unobserved, on a
        copy of ``y``.  ``superob`` (``_superob_setting``, dense mode): not None = the kept observations are merged into
        superobservations ahead of the analysis; the ``observed`` mask stays the raw one.  ``regions`` (dense mode): a label
        map; ``info["regions"]`` then holds the regional means and their exact errors (``dense.OI_dense``).  ``fit_scale``
        (``_scale_setting``, dense mode): not None = the knee scale is only the starting point of a maximum-likelihood fit of the
        error scales; ``info["scale"]`` is then knee x scale_b, beside ``scale_knee``, ``scale_fit`` and ``likelihood``.
        ``ensemble`` (``_ensemble_setting``, dense mode): not None = ``(K, F)``, and ``info["ensemble"]`` holds K posterior draws.
        ``drift`` (``_drift_setting``, dense mode): not None = the degree of the drift estimated with the analysis; ``info["drift"]``."""
        from . import dense
        from . import optimal_interpolation as oi_mod
        index, scale, curve, found = oi_mod.regularization_pick(Sa, So, reg_index)
        print("The regularization factor is " + str(scale))
        corr_fit = None
        if isinstance(L, str):                                   # "auto": the length the month's own innovations support
            corr_fit = dense.estimate_corr_length(xa, y, Sa, So, lat, lon, scale=scale, corr=corr)
            corr_fit.pop("covariogram", None)
            if corr_fit["found"]:
                L = float(corr_fit["L_km"])
            else:                                                # (the knee_found convention: say so once, use the default)
                L = 300.0
                print("No correlation length could be fitted to the innovations; using 300 km")
        qc_info = qc_mask = None
        if qc is not None:
            res = dense.qc_innovations(xa, y, Sa, So, lat, lon, L, scale=scale, corr=corr, **qc)
            qc_mask = res["rejected_cells"]
            qc_info = {"method": "buddy", "nrejected": int(res["rejected"].sum()),
                       "n_background": int((res["reason"] == dense.QC_BACKGROUND).sum()),
                       "n_buddy": int((res["reason"] == dense.QC_BUDDY).sum()), "passes": res["passes"],
                       "k_background": res["k_background"], "k_buddy": res["k_buddy"], "min_buddies": res["min_buddies"],
                       "cmin": res["cmin"], "L_km": res["L_km"]}
            print(f"Quality control rejected {qc_info['nrejected']} of {res['rejected'].size} observations")
            y = np.array(y, dtype=np.float64)                    # a copy: the rejected cells are unobserved from here on
            y[qc_mask] = np.nan
            if corr_fit is not None:                             # "auto": the analysis' length is the one the kept observations support
                qc_info["corr_fit_before"] = corr_fit
                corr_fit = dense.estimate_corr_length(xa, y, Sa, So, lat, lon, scale=scale, corr=corr)
                corr_fit.pop("covariogram", None)
                if corr_fit["found"]:
                    L = float(corr_fit["L_km"])
                else:
                    L = 300.0
                    print("No correlation length could be fitted to the kept innovations; using 300 km")
        if mode == "dense":
            xb, inc, info = dense.OI_dense(xa, y, Sa, So, lat, lon, L, scale=scale, want_error=want_error, corr=corr,
                                           nprobe=nprobe or 256, superob=superob, regions=regions, fit_scale=fit_scale,
                                           **({} if ensemble is None else {"ensemble": ensemble[0], "ensemble_features": ensemble[1]}),
                                           **({} if drift is None else {"drift": drift}))
            if fit_scale is not None:
                fit = info["scale_fit"]
                print(f"The maximum-likelihood error scales are {fit['scale_b']:g} (background) and {fit['scale_o']:g} (observations)"
                      + ("" if fit["found"] else "; no fit was made"))
            so = info.get("superob")
            if so is not None and so["box_deg"] * dense.KM_PER_DEG > 0.5 * L:      # (the knee_found convention: say so once)
                print(f"The superobservation box of {so['box_deg']:g} degrees ({so['box_deg'] * dense.KM_PER_DEG:.0f} km) is wider "
                      f"than half the correlation length ({L:g} km)")
        else:
            xb, inc, info = dense.OI_tiled(xa, y, Sa, So, lat, lon, L, tile_deg=tile, scale=scale, want_error=want_error, corr=corr)
        xb, inc = np.array(xb, dtype=np.float64), np.array(inc, dtype=np.float64)
        if want_error:
            err, ak = np.array(info["err"], dtype=np.float64), np.array(info["ak"], dtype=np.float64)
        else:        # posterior error and averaging kernel cost n m^2 flop (1e16 at 720x1440 / 1e5 obs): skipped on request
            err, ak = np.full(xb.shape, np.nan), np.full(xb.shape, np.nan)
        # cells the reference's OI gives numbers for: y, So, xa, Sa all non-NaN.  So = +inf there means K = 0 (no weight):
        # the dense analysis simply does not use such an observation, and AK = 0 as in the reference; Sa*reg = 0 makes the
        # reference's AK = 1 - Sb/(Sa*reg) a 0/0 (optimal_interpolation.py:31): mirrored.
        observed = np.isfinite(y) & ~np.isnan(So) & np.isfinite(xa) & np.isfinite(Sa)
        scale_knee = scale
        if fit_scale is not None:                               # from here on the scale is the analysis' own
            scale = scale * info["scale_fit"]["scale_b"]
        if want_error:
            ak[observed & np.isinf(So)] = 0.0
            ak[observed & (Sa * scale == 0)] = np.nan
        if unobserved == "nan":
            for a in (xb, inc, err, ak):
                a[~observed] = np.nan
        else:
            if want_error:
                ak[~observed & np.isfinite(xa)] = 0.0
            for a in (inc, err, ak):
                a[~np.isfinite(xa)] = np.nan
        out_info = {"mode": mode, "corr_length_km": L, "correlation": corr, "scale": scale, "reg_index": index, "knee_found": found,
                    "nobs": info["nobs"], "unobserved": unobserved, "want_error": want_error}
        if want_error == "mc":                                  # the estimate's own standard errors travel with it
            out_info.update(error_method="mc", nprobe=info["nprobe"], err_se=info["err_se"], ak_obs_se=info["ak_obs_se"])
        if corr_fit is not None:
            out_info["corr_fit"] = corr_fit
        if qc_info is not None:
            out_info["qc"], out_info["qc_rejected"] = qc_info, qc_mask
        if info.get("superob") is not None:
            out_info["superob"] = info["superob"]
        if info.get("regions") is not None:
            out_info["regions"] = info["regions"]
        if info.get("ensemble") is not None:
            out_info["ensemble"] = info["ensemble"]
        if info.get("drift") is not None:
            out_info["drift"] = info["drift"]
        if fit_scale is not None:
            out_info.update(scale_knee=scale_knee, scale_fit=info["scale_fit"], likelihood=info["likelihood"])
        return (xb, ak, inc, err), out_info

    def scaling_factor(self):
        """posterior / prior model column with NaN, inf and 0 mapped to 1.0 -- the field the downstream
        emission tools consume (write_to_nc, driver.py:204-206); evaluated on the device."""
        post = np.ascontiguousarray(self.ctm_averaged_vcd_corrected)
        prior = np.ascontiguousarray(self.ctm_averaged_vcd)
        ctx = _hip.context()
        dt = _hip.compute_dtype(post, prior)
        n = int(post.size)
        buf = ctx.alloc(3 * n * dt.itemsize)
        ctx.upload_into(buf.at(0), post, dtype=dt)
        ctx.upload_into(buf.at(n * dt.itemsize), prior, dtype=dt)
        ctx.check(ctx.lib.oisat_scaling_factor(ctx.h, _hip.dtype_code(dt), buf.at(0), buf.at(n * dt.itemsize), n,
                                               buf.at(2 * n * dt.itemsize)))
        return ctx.download(buf.at(2 * n * dt.itemsize), post.shape, dt)

    def output_fields(self):
        """The variables of the reference's output file, in its order and as float32 (driver.py:179-225)."""
        lon, lat = self._first_granule_grid()
        f32 = lambda a: np.asarray(a, dtype=np.float32)       # noqa: E731
        return {
            "sat_averaged_vcd": f32(self.sat_averaged_vcd), "ctm_averaged_vcd_prior": f32(self.ctm_averaged_vcd),
            "ctm_averaged_vcd_posterior": f32(self.ctm_averaged_vcd_corrected), "sat_averaged_error": f32(self.sat_averaged_error),
            "ak_OI": f32(self.ak_OI), "error_OI": f32(self.error_OI), "scaling_factor": f32(self.scaling_factor()),
            "lon": f32(lon), "lat": f32(lat), "aux1": f32(self.aux1), "aux2": f32(self.aux2),
        }

    def write_to_nc(self, output_file, output_folder='diag'):
        '''
        Write the final results to a netcdf (same variable names, types and dimensions as the reference,
        driver.py:156-227).  Uses netCDF4 when it is installed; otherwise SciPy's NetCDF-3 writer.
        ``output_file``: file name without the extension; ``output_folder`` is created when missing.
        '''
        if not os.path.exists(output_folder):
            os.makedirs(output_folder)
        fields = self.output_fields()
        path = output_folder + '/' + output_file + '.nc'
        time_string = self.avg_time.strftime("%Y-%m-%d %H:%M:%S")
        nx_, ny_ = np.shape(self.sat_averaged_vcd)[0], np.shape(self.sat_averaged_vcd)[1]
        try:
            from netCDF4 import Dataset
        except ImportError:
            Dataset = None
        if Dataset is not None:
            nc = Dataset(path, 'w')
            nc.createDimension('x', nx_)
            nc.createDimension('y', ny_)
            nc.createDimension('t', None)
            tv = nc.createVariable('time', 'S1', ('t'))
            tv[:] = np.array(list(time_string), 'S1')
            for name, arr in fields.items():
                v = nc.createVariable(name, 'f4', ('x', 'y'))
                v[:, :] = arr
            nc.close()
        else:
            from scipy.io import netcdf_file
            nc = netcdf_file(path, 'w')
            nc.createDimension('x', nx_)
            nc.createDimension('y', ny_)
            nc.createDimension('t', len(time_string))       # NetCDF-3 via SciPy: fixed length instead of unlimited
            tv = nc.createVariable('time', 'c', ('t',))
            tv[:] = np.array(list(time_string), 'S1')
            for name, arr in fields.items():
                v = nc.createVariable(name, 'f', ('x', 'y'))
                v[:, :] = arr
            nc.close()
        return path

    # ---- outside the hot path ---------------------------------------------------------------
    def _out_of_scope(self, name):
        raise NotImplementedError(
            f"oisatgmi.{name} (file I/O / sensor operators / reporting) is outside the MI355X hot path; "
            f"use the reference implementation for it and bind this package for average/bias_correct/oi "
            f"(INTEGRATION.md)")

    def read_data(self, *a, **k):
        self._out_of_scope("read_data")

    def recal_amf(self):
        from .amf_recal import amf_recal
        self.reader_obj.sat_data = amf_recal(self.reader_obj.ctm_data, self.reader_obj.sat_data)

    def cal_pwv(self):
        """driver.py:42-44 of the reference."""
        from .pwv_cal import pwv_calculator
        self.reader_obj.sat_data = pwv_calculator(self.reader_obj.ctm_data, self.reader_obj.sat_data)

    def conv_ak(self, sensor: str):
        """driver.py:46-51 of the reference."""
        if sensor == 'MOPITT':
            from .ak_conv_mopitt import ak_conv_mopitt
            self.reader_obj.sat_data = ak_conv_mopitt(self.reader_obj.ctm_data, self.reader_obj.sat_data)
        if sensor == 'GOSAT':
            from .ak_conv_gosat import ak_conv_gosat
            self.reader_obj.sat_data = ak_conv_gosat(self.reader_obj.ctm_data, self.reader_obj.sat_data)

    def reporting(self, *a, **k):
        self._out_of_scope("reporting")

    def savedaily(self, folder, gasname, date):
        """Per-granule .mat dumps (driver.py:135-155 of the reference): host-side file writing only, same file names
        and variable names; kept so that run/job.py's ``save_daily`` switch works with this facade."""
        from scipy.io import savemat
        if not os.path.exists(folder):
            os.makedirs(folder)
        first_valid_idx = next(i for i, sat_data in enumerate(self.reader_obj.sat_data) if sat_data is not None)
        latitude = self.reader_obj.ctm_data[first_valid_idx].latitude
        longitude = self.reader_obj.ctm_data[first_valid_idx].longitude
        for counter, sat in enumerate(self.reader_obj.sat_data):
            if sat is None:
                continue
            time_sat = 10000.0 * sat.time.year + 100.0 * sat.time.month + sat.time.day + sat.time.hour / 24.0
            savemat(folder + "/" + "sat_data_" + gasname + "_" + str(time_sat) + str(counter) + ".mat",
                    {"vcd_sat": sat.vcd, "vcd_ctm": sat.ctm_vcd, "vcd_err": sat.uncertainty, "time_sat": time_sat,
                     "lat": latitude, "lon": longitude})

