"""Drop-in surface: the reference's labelled-array API over the HIP engine.

Same names, positional order, defaults and return conventions as

    LagrangianCoherence.LCS.LCS.LCS                       LCS/LCS.py:19-168
    LagrangianCoherence.LCS.LCS.flowmap_gradient          LCS/LCS.py:171-225
    LagrangianCoherence.LCS.trajectory.parcel_propagation LCS/trajectory.py:8-144

xarray in, xarray out.  The adapter touches only ``dims``, ``values``, coordinates and ``name`` and returns
results in the class of its inputs, so where xarray is not installed (this image) the same code runs on any
duck-typed labelled array (the tests use the stand-in of tests/labelled.py; nothing here imports it).  All arithmetic happens in the
HIP library; this file is argument handling only.

Deliberate differences from the reference (all outside the arithmetic):
  * the unconditional ``print('!'*100)`` and ``print('using s = ...')`` (LCS.py:74,126)
    are not reproduced; ``verbose`` prints the same progress lines;
  * ``isglobal=True`` runs the 0.5 degree regrid and the T20 spectral truncation on the
    device (``preprocess.py``); the truncation restates windspharm/SPHEREPACK's published
    algorithm in float64 and is NOT pinned against pyspharm (not installable here);
  * ``cyclic_xboundary=False`` (the default of both call forms) reproduces the reference's clamp as it is
    written -- outer-product assignment over offending rows x columns (LCS/trajectory.py:96-97):
    the fused kernel runs first and, only if a parcel really left the longitude range, the engine re-runs
    sub-step by sub-step with that rule (``lc_advect`` mode ``LC_X_CLAMP_REFERENCE_OUTER``);
  * mixed float32/float64 inputs are computed in float64 (engine.common_dtype);
  * float64 calls of up to 2^18 seeds (the example's 89 x 180 grid, the 360 x 721 common grid of ``isglobal=True``)
    follow numpy / scipy's operation order (LCS/trajectory.py:86-87,110-112): ~1e-13 degrees from the reference.
    Larger float64 calls take the fused-level form, which differs by rounding only (<= 1e-9 degrees, or the flow's own
    response to a 1e-12 degree seed shift where that is larger); ``get_engine().set_f64_fidelity('exact' | 'fast' |
    'auto')`` chooses explicitly (INTEGRATION.md "Behavioural notes").
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from .engine import Engine, _smoothing_width, common_dtype

__all__ = ["LCS", "parcel_propagation", "flowmap_gradient", "get_engine"]

_ENGINE = None


def get_engine() -> Engine:
    """Process-wide engine on the current torch device (created on first use)."""
    global _ENGINE
    if _ENGINE is None:
        _ENGINE = Engine()
    return _ENGINE


# ---------------------------------------------------------------------------
# labelled-array adapter
# ---------------------------------------------------------------------------
def _is_xarray(obj) -> bool:
    return type(obj).__module__.split(".")[0] == "xarray"


def _make(like, data, dims, coords, name=None):
    if _is_xarray(like):
        import xarray as xr
        return xr.DataArray(data, dims=dims, coords=coords, name=name)
    # any other labelled-array class: results come back in the class they came in (constructor (data, dims, coords,
    # name); the tests' xarray-free stand-in, tests/labelled.py, is one)
    return type(like)(data, dims, coords, name)


def _resample_linear(da, dim, freq):
    """``da.resample({dim: freq}).interpolate('linear')`` (LCS/LCS.py:89-90) for a labelled array that is not an
    xarray object: the new time axis is pandas' resampling index of the old one (what xarray's grouper calls
    ``full_index``), the values go through ``scipy.interpolate.interp1d(kind='linear', bounds_error=False)`` on the
    times as float64 nanoseconds since the first one -- the two kernels xarray itself delegates to."""
    import pandas as pd
    from scipy.interpolate import interp1d
    t = pd.DatetimeIndex(np.asarray(da.coords[dim]))
    full = pd.Series(np.arange(t.size), index=t).resample(freq).asfreq().index
    t0 = t.values.astype("datetime64[ns]").min()
    x = (t.values.astype("datetime64[ns]") - t0).astype("int64").astype(np.float64)
    xn = (full.values.astype("datetime64[ns]") - t0).astype("int64").astype(np.float64)
    ax = list(da.dims).index(dim)
    vals = interp1d(x, np.asarray(da.values), kind="linear", axis=ax, bounds_error=False, assume_sorted=True)(xn)
    coords = dict(da.coords)
    coords[dim] = full.values
    return type(da)(vals, da.dims, coords, getattr(da, "name", None))


def _coord(da, dim):
    return np.asarray(da[dim].values)


def _sorted_tll(da, timedim):
    """values as (time, latitude, longitude) with lat/lon ascending, plus the coordinates.

    The reference sorts with ``sortby`` (trajectory.py:49-52, LCS.py:101-104)."""
    vals = np.asarray(da.transpose(timedim, "latitude", "longitude").values)
    lat, lon, time = _coord(da, "latitude"), _coord(da, "longitude"), _coord(da, timedim)
    ilat, ilon = np.argsort(lat, kind="stable"), np.argsort(lon, kind="stable")
    if not np.array_equal(ilat, np.arange(lat.size)):
        vals, lat = vals[:, ilat, :], lat[ilat]
    if not np.array_equal(ilon, np.arange(lon.size)):
        vals, lon = vals[:, :, ilon], lon[ilon]
    return vals, time, lat, lon


def _to_np(t):
    return get_engine().to_host(t)


# ---------------------------------------------------------------------------
# trajectory.parcel_propagation
# ---------------------------------------------------------------------------
def _check_tracer(C, U, u_time, lat, lon, propdim):
    """The tracer's values as (time, latitude, longitude) after sorting, checked against U's dims and coordinates."""
    assert set(C.dims) == set(U.dims), "C and U dims are different"
    c, c_time, c_lat, c_lon = _sorted_tll(C, propdim)
    assert np.array_equal(c_time, u_time) and np.array_equal(c_lat, lat) and np.array_equal(c_lon, lon), \
        "C coordinates differ from U coordinates"
    return c


def parcel_propagation(U, V, timestep=1, propdim="time", verbose=True, return_traj=False, SETTLS_order=0,
                       copy=False, interp_order=3, cyclic_xboundary=False, C=None):
    """Lagrangian 2-time-level advection.  Signature of LCS/trajectory.py:8-18.

    Returns ``(positions_x, positions_y)``: 2-D ``(latitude, longitude)`` arrays with a
    scalar ``propdim`` coordinate equal to the last entry of the (possibly reversed)
    time list (trajectory.py:141-142), or with ``return_traj`` 3-D
    ``(propdim, latitude, longitude)`` arrays whose entry 0 is the seed grid
    (trajectory.py:73-74,138-139).

    ``C``: a scalar tracer on U's grid and time levels (the call LCS/area_of_influence.py:314-316 makes; the dead flag
    ``tracer_account`` of trajectory.py:45).  Returns ``(positions_x, positions_y, c)``: ``c`` has ``positions_x``'s dims
    and labels, entry i the tracer at time level i (stored order, Q6) sampled at trajectory entry i with the call's
    ``interp_order`` (tools.xr_map_coordinates); without ``return_traj`` the last entry.  ``c.mean(propdim)`` is the
    driver's ``c_int``.  Positions are bit-identical to the call without ``C``.
    """
    verboseprint = print if verbose else (lambda *a, **k: None)
    u, time, lat, lon = _sorted_tll(U, propdim)
    v, _, _, _ = _sorted_tll(V, propdim)
    c = None if C is None else _check_tracer(C, U, time, lat, lon, propdim)
    times = time.tolist()                                   # trajectory.py:58
    if timestep < 0:
        times.reverse()                                     # labels only (Q6)
    eng = get_engine()
    verboseprint(f"Propagating {len(times) - 1} time levels on {eng.device}")
    # pack + advect in one call (large float64 order-3 series: the pack of chunk k+1 overlaps the advect of chunk k)
    res = eng.pack_and_advect(u, v, lat, lon, lat, lon, timestep, SETTLS_order=SETTLS_order, interp_order=interp_order,
                              cyclic_xboundary=cyclic_xboundary, return_traj=return_traj,
                              fuse_levels=eng.f64_fuse_levels(common_dtype(u, v, lat, lon), lat.size * lon.size))
    field, res = res[0], res[1:]
    cs = None
    if c is not None:
        # the tracer in the field's compute dtype, sampled along the positions just computed (entry i at level i)
        tracer = eng.prepare_tracer(c, None, lat, lon, interp_order, dtype=field.dtype)
        if return_traj:
            cs = eng.sample_tracer(tracer, res[2], res[3], 0, interp_order)[0][0]
        else:
            cs = eng.sample_tracer(tracer, res[0][None], res[1][None], field.nt - 1, interp_order)[0][0][0]
    coords2d = {"latitude": lat, "longitude": lon}
    if return_traj:
        assert type(times[0]).__name__ != "Datetime360Day", \
            'Cannot return trajectories with time cooridnates cftime.Datetime360Day.'   # trajectory.py:129-130
        import pandas as pd
        tindex = pd.Index(pd.to_datetime(times), name=propdim)                          # trajectory.py:138
        tcoord = tindex if _is_xarray(U) else np.asarray(tindex.values)
        dims = (propdim, "latitude", "longitude")
        px = _make(U, _to_np(res[2]), dims, {propdim: tcoord, **coords2d}, getattr(U, "name", None))
        py = _make(U, _to_np(res[3]), dims, {propdim: tcoord, **coords2d}, getattr(U, "name", None))
        if cs is not None:
            return px, py, _make(U, _to_np(cs), dims, {propdim: tcoord, **coords2d}, getattr(C, "name", None))
        return px, py
    dims = ("latitude", "longitude")
    px = _make(U, _to_np(res[0]), dims, {**coords2d, propdim: times[-1]}, getattr(U, "name", None))
    py = _make(U, _to_np(res[1]), dims, {**coords2d, propdim: times[-1]}, getattr(U, "name", None))
    if cs is not None:
        return px, py, _make(U, _to_np(cs), dims, {**coords2d, propdim: times[-1]}, getattr(C, "name", None))
    return px, py


# ---------------------------------------------------------------------------
# LCS.flowmap_gradient
# ---------------------------------------------------------------------------
def flowmap_gradient(x_departure, y_departure, sigma=None):
    """The 9-component deformation tensor, dims ``(derivatives, latitude, longitude)``.
    Signature of LCS/LCS.py:171."""
    lat, lon = _coord(x_departure, "latitude"), _coord(x_departure, "longitude")
    x = np.asarray(x_departure.transpose("latitude", "longitude").values)
    y = np.asarray(y_departure.transpose("latitude", "longitude").values)
    ilat, ilon = np.argsort(lat, kind="stable"), np.argsort(lon, kind="stable")   # tools.py:250-251
    x, y, lat, lon = x[ilat][:, ilon], y[ilat][:, ilon], lat[ilat], lon[ilon]
    dtype = common_dtype(x, y, lat, lon)
    lat_t, lon_t = lat.astype(dtype), lon.astype(dtype)
    eng = get_engine()
    xd, yd = eng.to_device(x, dtype), eng.to_device(y, dtype)
    if isinstance(sigma, (float, int)) and sigma > 1e-15:                          # LCS.py:187-190
        xd, yd = eng.gaussian_filter(xd, sigma), eng.gaussian_filter(yd, sigma)
    dt = eng.flowmap_gradient(xd, yd, lat_t, float(lat_t[1] - lat_t[0]), float(lon_t[1] - lon_t[0]))
    names = ["dxdx", "dxdy", "dydx", "dydy", "dzdx", "dzdy", "dxdr", "dydr", "dzdr"]   # LCS.py:210-220
    return _make(x_departure, _to_np(dt), ("derivatives", "latitude", "longitude"),
                 {"derivatives": np.array(names), "latitude": lat, "longitude": lon})


# ---------------------------------------------------------------------------
# LCS.LCS
# ---------------------------------------------------------------------------
def _crop_strict(lat, lon, sub):
    """Row/column masks of ``latlonsel`` with strict inequalities (LCS/tools.py:158-187)."""
    def bounds(s):
        if isinstance(s, slice):
            return s.start, s.stop
        return s[0], s[-1]
    la = bounds(sub.get("latitude", sub.get("lat")))
    lo = bounds(sub.get("longitude", sub.get("lon")))
    mlat = np.ones(lat.shape, bool) if la[0] is None else (lat > la[0])
    mlat &= np.ones(lat.shape, bool) if la[1] is None else (lat < la[1])
    mlon = np.ones(lon.shape, bool) if lo[0] is None else (lon > lo[0])
    mlon &= np.ones(lon.shape, bool) if lo[1] is None else (lon < lo[1])
    return mlat, mlon


# Engine.lcs_aux's form of each windowed engine method (LCS._run_windows with aux_grid)
_AUX_FORMS = {"lcs_series": dict(n_dirs=1, want=("sigma",)), "lcs_bidirectional": dict(n_dirs=2, want=("sigma",)),
              "lcs_strain": dict(n_dirs=1, want=("s1", "s2", "e_lon", "e_lat"))}


class _Record(NamedTuple):
    """One record as :meth:`LCS._record_intake` hands it to the engine calls and to the labelling of their results."""
    like: object            # the caller's u (resampled): results come back in its class
    uu: np.ndarray          # (time, latitude, longitude), latitude and longitude ascending
    vv: np.ndarray
    time: np.ndarray
    lat: np.ndarray
    lon: np.ndarray
    timestep: float         # signed; with ``resample`` the resampled spacing in seconds
    cyclic_xboundary: bool
    n_windows: int
    wlen: int               # levels of the sorted record in one window
    wstep: int              # levels between the starts of two windows


class LCS:
    """API to compute the Finite-time Lyapunov exponent in 2D wind fields (LCS/LCS.py:19-46).

    Returns sigma_max, the largest singular value of the reference's deformation
    tensor; FTLE is the caller's ``log(sigma)/2`` (examples/ideal_vortex.py:282,288).
    """
    earth_r = 6371000  # metres

    def __init__(self, timestep: float = 1, timedim='time', SETTLS_order=0, subdomain=None, return_dpts=False,
                 gauss_sigma=None, aux_grid=None):
        """The reference's arguments (LCS/LCS.py:25-27), then ``aux_grid`` (pass it by keyword): ``None`` is the reference's
        gradient, the 5-point stencil over neighbouring output points; a positive number of degrees takes the flow-map
        gradient of every call form from an auxiliary grid instead -- four extra parcels per output point, offset by that much
        east, west, north and south (``Engine.lcs_aux``; INTEGRATION.md "Auxiliary-grid FTLE").  Same labelled results; cells
        within ``aux_grid`` of the field's edge are NaN.  Not together with ``gauss_sigma``."""
        if aux_grid is not None:
            if isinstance(aux_grid, bool) or not isinstance(aux_grid, (int, float, np.integer, np.floating)) \
                    or not np.isfinite(aux_grid) or aux_grid <= 0:
                raise ValueError(f"aux_grid {aux_grid!r}: a positive, finite offset in degrees (or None)")
            if _smoothing_width(gauss_sigma) > 1e-15:
                raise ValueError("aux_grid and gauss_sigma: smoothing departure fields across seeds contradicts the auxiliary "
                                 "grid's local gradient; use one or the other")
            aux_grid = float(aux_grid)
        self.timestep = timestep
        self.SETTLS_order = SETTLS_order
        self.timedim = timedim
        self.subdomain = subdomain
        self.gauss_sigma = gauss_sigma
        self.return_dpts = return_dpts
        self.aux_grid = aux_grid

    def __call__(self, ds=None, u=None, v=None, verbose=True, s=None, resample=None, s_is_error=False,
                 isglobal=False, return_traj=False, interp_to_common_grid=True, traj_interp_order=3, truncation=20):
        verboseprint = print if verbose else (lambda *a, **k: None)
        timedim = self.timedim
        rec = self._record_intake(ds, u, v, None, 1, resample, isglobal, interp_to_common_grid, truncation, verbose)
        lat, lon = rec.lat, rec.lon
        eng = get_engine()

        verboseprint("*---- Parcel propagation ----*")
        dtype = common_dtype(rec.uu, rec.vv, lat, lon)
        lat_t, lon_t = lat.astype(dtype), lon.astype(dtype)
        if self.aux_grid is not None:
            res = self._call_aux(eng, rec, lat_t, lon_t, dtype, traj_interp_order, return_traj)
        else:
            res = eng.lcs_wind(rec.uu, rec.vv, lat, lon, lat_t, lon_t, rec.timestep, SETTLS_order=self.SETTLS_order,
                               interp_order=traj_interp_order, cyclic_xboundary=rec.cyclic_xboundary,
                               fuse_levels=eng.f64_fuse_levels(dtype, lat.size * lon.size),
                               gauss_sigma=self.gauss_sigma, return_traj=return_traj)          # LCS.py:129-154
        verboseprint("*---- Done eigenvalues ----*")

        forward = np.sign(rec.timestep) == 1
        eigenvalues = self._windows_out(rec, forward, _to_np(res["sigma"])[None], getattr(rec.like, "name", None))  # LCS.py:159-160
        times = rec.time.tolist()
        if rec.timestep < 0:
            times.reverse()

        def dep(k):
            return self._departure_out(rec, _to_np(res[k]), rec.timestep < 0)

        def traj(k):
            import pandas as pd
            tindex = pd.Index(pd.to_datetime(times), name=timedim)
            tcoord = tindex if _is_xarray(rec.like) else np.asarray(tindex.values)
            return _make(rec.like, _to_np(res[k]), (timedim, "latitude", "longitude"),
                         {timedim: tcoord, "latitude": lat, "longitude": lon})

        if self.return_dpts and return_traj:                               # LCS.py:161-168
            return eigenvalues, dep("x_dep"), dep("y_dep"), traj("traj_x"), traj("traj_y")
        elif self.return_dpts:
            return eigenvalues, dep("x_dep"), dep("y_dep")
        elif return_traj:
            return eigenvalues, traj("traj_x"), traj("traj_y")
        return eigenvalues

    def series(self, ds=None, u=None, v=None, window=None, stride=1, verbose=True, s=None, resample=None, s_is_error=False,
               isglobal=False, interp_to_common_grid=True, traj_interp_order=3, truncation=20):
        """sigma_max over sliding windows of one record in one call: what the loop of LCS/area_of_influence.py:168-181 makes
        of ``LCS(...)(ds.isel(time=np.arange(w * stride, w * stride + window)), ...)``.

        ``window`` and ``stride`` count time levels of the record as given (before ``resample``); window ``w`` is the levels
        ``[w * stride, w * stride + window)`` and there are ``(nt - window) // stride + 1`` of them.  Entry ``w`` of the result
        is what the call on that slice returns (its time label included: the window's last time going forward, its first
        going backward); the result has dims ``(timedim, latitude, longitude)``, and with ``return_dpts`` ``x_dep`` / ``y_dep``
        get the same leading time dimension.  Sorting, ``resample`` (linear in time between original levels, so resampling
        the record and slicing it gives what resampling each slice gives, except at a slice's first level: see below), the 0.5 degree regrid and the T20 truncation
        (both level by level) run once on the whole record (:meth:`_record_intake`); the record is packed once and every window
        is advected in one batched call (``Engine.lcs_series``).  Two places where the windows agree with the per-window calls
        to rounding, not bit for bit: float64 at order 3 on grids of 256 rows or more (a level packed with the whole record may differ
        in its last bits from the same level packed inside one window: the pack cuts levels into row pieces by the number
        of levels), and -- with ``resample`` -- the first level of every window after the first: the per-window call's
        interpolation returns the original level there, the record's the left interval's value, which can differ in the
        last bit of the input."""
        verboseprint = print if verbose else (lambda *a, **k: None)
        if window is None:                                                 # (the intake's one-window form is not a series)
            raise ValueError(f"window {window!r}: at least 2 time levels")
        rec = self._record_intake(ds, u, v, window, stride, resample, isglobal, interp_to_common_grid, truncation, verbose)
        verboseprint(f"*---- Parcel propagation: {rec.n_windows} windows ----*")
        res = self._run_windows("lcs_series", rec, rec.timestep, traj_interp_order)
        verboseprint("*---- Done eigenvalues ----*")

        forward = np.sign(rec.timestep) == 1
        eigenvalues = self._windows_out(rec, forward, _to_np(res["sigma"]), getattr(rec.like, "name", None))
        if self.return_dpts:                                               # LCS.py:161-168
            return (eigenvalues, self._windows_out(rec, forward, _to_np(res["x_dep"]), crop=False),
                    self._windows_out(rec, forward, _to_np(res["y_dep"]), crop=False))
        return eigenvalues

    def bidirectional(self, ds=None, u=None, v=None, window=None, stride=1, verbose=True, s=None, resample=None,
                      s_is_error=False, isglobal=False, interp_to_common_grid=True, traj_interp_order=3, truncation=20):
        """The attracting and the repelling field of one record in one call: ``(attracting, repelling)``, what the reference's
        example computes with two calls (examples/ideal_vortex.py:280-288).

        ``window=None``: ``attracting`` is what ``LCS(timestep=-abs(timestep), same ctor args)(ds, same call args)`` returns
        and ``repelling`` the same with ``+abs(timestep)`` (values, dims, the time labels of LCS.py:158 and the tuple of
        ``return_dpts``).  ``window=k``: the same against ``.series(ds, window=k, stride=stride, ...)`` for each sign.
        Sorting, ``resample``, the regrid and T20 (:meth:`_record_intake`) and the pack run once; then one
        ``lc_advect_series_dirs`` call and one ``lc_sigma_batch`` call per memory group (``Engine.lcs_bidirectional``).  The levels
        are read in stored order in both directions, so both directions advect over the same packed record.  Bit-identical to the
        single-direction calls except where :meth:`series` is not (its docstring): with ``window=None`` only float64 order 3
        on grids of 256 rows or more can differ, to rounding."""
        verboseprint = print if verbose else (lambda *a, **k: None)
        if not self.timestep:
            raise ValueError(f"timestep {self.timestep!r}: bidirectional needs a non-zero step (its sign is ignored)")
        rec = self._record_intake(ds, u, v, window, stride, resample, isglobal, interp_to_common_grid, truncation, verbose)
        verboseprint(f"*---- Parcel propagation: {rec.n_windows} window(s), both directions ----*")
        res = self._run_windows("lcs_bidirectional", rec, abs(rec.timestep), traj_interp_order)
        verboseprint("*---- Done eigenvalues ----*")

        sig_all = _to_np(res["sigma"])
        x_all, y_all = (_to_np(res[k]) for k in ("x_dep", "y_dep")) if self.return_dpts else (None, None)
        out = []
        for d, forward in ((0, False), (1, True)):
            eigenvalues = self._windows_out(rec, forward, sig_all[d], getattr(rec.like, "name", None))
            if not self.return_dpts:
                out.append(eigenvalues)
            elif window is None:                                           # as __call__: (lat, lon) with a scalar time label
                out.append((eigenvalues, self._departure_out(rec, x_all[d, 0], not forward),
                            self._departure_out(rec, y_all[d, 0], not forward)))
            else:                                                          # as series
                out.append((eigenvalues, self._windows_out(rec, forward, x_all[d], crop=False),
                            self._windows_out(rec, forward, y_all[d], crop=False)))
        return tuple(out)

    def _record_intake(self, ds, u, v, window, stride, resample, isglobal, interp_to_common_grid, truncation, verbose) -> _Record:
        """What every call form does with its record before the engine sees it: intake (LCS.py:81-96), the window / stride
        checks, ``resample`` on the whole record (LCS.py:88-91), sort (LCS.py:101-104), the 0.5 degree regrid and the T20
        truncation (LCS.py:106-118).  ``window=None``: one window, the whole (resampled) record, as ``__call__`` takes it."""
        timedim = self.timedim
        self.verbose = verbose
        if window is not None:
            if isinstance(window, bool) or int(window) != window or int(window) < 2:
                raise ValueError(f"window {window!r}: at least 2 time levels")
            if isinstance(stride, bool) or int(stride) != stride or int(stride) < 1:
                raise ValueError(f"stride {stride!r}: at least 1 time level")
            window, stride = int(window), int(stride)
        if isinstance(ds, str):                                            # LCS.py:84-87
            import xarray as xr
            ds = xr.open_dataset(ds)
        if ds is not None and not isinstance(ds, str):                     # LCS.py:81-83
            u = ds.u.copy()
            v = ds.v.copy()
        assert set(u.dims) == set(v.dims), "u and v dims are different"                     # LCS.py:95
        assert set(u.dims) == {'latitude', 'longitude', timedim}, \
            'array dims should be latitude and longitude only'                             # LCS.py:96
        if window is not None:
            t_orig = np.asarray(u[timedim].values)
            nt = t_orig.size
            if window > nt:
                raise ValueError(f"window {window} is longer than the record ({nt} time levels)")
        timestep = self.timestep
        r = 1
        if isinstance(resample, str):                                      # LCS.py:88-91, on the whole record
            if _is_xarray(u):
                u = u.resample({timedim: resample}).interpolate('linear')
                v = v.resample({timedim: resample}).interpolate('linear')
            else:
                u = _resample_linear(u, timedim, resample)
                v = _resample_linear(v, timedim, resample)
            t_new = np.asarray(u[timedim].values)
            if window is not None:
                r = _resample_ratio(t_orig, t_new)
            timestep = np.sign(timestep) * (t_new[1] - t_new[0]).astype('timedelta64[s]').astype('float')

        uu, time, lat, lon = _sorted_tll(u, timedim)                       # LCS.py:101-104
        vv, _, _, _ = _sorted_tll(v, timedim)
        if window is None:                                                 # one window: the whole (resampled) record
            n_windows, wlen, wstep = 1, int(time.size), 1
        else:
            n_windows = (nt - window) // stride + 1
            wlen, wstep = (window - 1) * r + 1, stride * r                # a window and the distance between two, in levels
        eng = get_engine()
        if isglobal:
            from . import preprocess
            if interp_to_common_grid:                                      # LCS.py:106-114
                uu, lat_new, lon_new = preprocess.regrid_common_grid(eng, uu, lat, lon)
                vv, _, _ = preprocess.regrid_common_grid(eng, vv, lat, lon)
                lat, lon = lat_new, lon_new
            if truncation is not None:                                     # LCS.py:115-118
                gridtype = preprocess.inspect_gridtype(lat)              # windspharm's: equally spaced global, or Gaussian
                uu = preprocess.spectral_truncate(eng, uu, truncation, gridtype)
                vv = preprocess.spectral_truncate(eng, vv, truncation, gridtype)
            self.subdomain = None                                          # LCS.py:119-120
        return _Record(u, uu, vv, time, lat, lon, timestep, bool(isglobal), n_windows, wlen, wstep)

    def _run_windows(self, method, rec: _Record, timestep, traj_interp_order):
        """Pack the record once -- the pack of the per-window call (Engine.lcs_wind -> pack_and_advect) -- and run the engine's
        ``method`` (``lcs_series``, ``lcs_bidirectional`` or ``lcs_strain``) over its windows."""
        eng = get_engine()
        field, lat_t, lon_t = self._packed_record(eng, rec, traj_interp_order)
        kw = dict(SETTLS_order=self.SETTLS_order, interp_order=traj_interp_order, cyclic_xboundary=rec.cyclic_xboundary,
                  gauss_sigma=self.gauss_sigma)
        if self.aux_grid is not None:
            # the same windows with the gradient of the auxiliary grid; the centre grid is advected only where it is returned
            return eng.lcs_aux(field, lat_t, lon_t, timestep, rec.wlen - 1, rec.n_windows, 0, rec.wstep, **kw, **_AUX_FORMS[method],
                               aux_delta=self.aux_grid, centre=bool(self.return_dpts))
        return getattr(eng, method)(field, lat_t, lon_t, timestep, rec.wlen - 1, rec.n_windows, 0, rec.wstep, **kw)

    def _packed_record(self, eng, rec: _Record, traj_interp_order):
        """The record packed once -- the pack of the per-window call (Engine.lcs_wind -> pack_and_advect) -- and the seed
        coordinates in its dtype: ``(field, lat, lon)``, what every windowed call form advects on."""
        lat, lon = rec.lat, rec.lon
        dtype = common_dtype(rec.uu, rec.vv, lat, lon)
        fuse, ext_image = eng._pack_options(dtype, self.SETTLS_order, eng.f64_fuse_levels(dtype, lat.size * lon.size), None)
        field = eng.prepare_field(rec.uu, rec.vv, lat, lon, traj_interp_order, fuse_levels=fuse, ext_image=ext_image)
        return field, lat.astype(dtype), lon.astype(dtype)

    def _call_aux(self, eng, rec: _Record, lat_t, lon_t, dtype, traj_interp_order, return_traj):
        """``__call__``'s engine work with ``aux_grid``: the departure points and trajectories of the output grid, where they are
        returned, by the call the reference's form makes (``Engine.pack_and_advect``: the same bits), and sigma from the
        auxiliary grid on the same packed field (``Engine.lcs_aux``)."""
        lat, lon = rec.lat, rec.lon
        fuse = eng.f64_fuse_levels(dtype, lat.size * lon.size)
        res = {}
        if self.return_dpts or return_traj:
            out = eng.pack_and_advect(rec.uu, rec.vv, lat, lon, lat_t, lon_t, rec.timestep, self.SETTLS_order, traj_interp_order,
                                      rec.cyclic_xboundary, fuse, None, None, return_traj, None)
            field = out[0]
            res["x_dep"], res["y_dep"] = out[1], out[2]
            if return_traj:
                res["traj_x"], res["traj_y"] = out[3], out[4]
        else:
            fuse, ext_image = eng._pack_options(dtype, self.SETTLS_order, fuse, None)
            field = eng.prepare_field(rec.uu, rec.vv, lat, lon, traj_interp_order, fuse_levels=fuse, ext_image=ext_image)
        aux = eng.lcs_aux(field, lat_t, lon_t, rec.timestep, field.nt - 1, 1, 0, 1, SETTLS_order=self.SETTLS_order,
                          interp_order=traj_interp_order, cyclic_xboundary=rec.cyclic_xboundary, gauss_sigma=self.gauss_sigma,
                          aux_delta=self.aux_grid)
        res["sigma"] = aux["sigma"][0]
        return res

    def _windows_out(self, rec: _Record, forward, a, name=None, crop=True, lead=None):
        """One result of an engine call, ``a`` with trailing axes (window, latitude, longitude), as a labelled array: the strict
        ``subdomain`` crop over the last two axes (LCS.py:143-144; ``crop=False``: departure points, which keep the whole grid),
        the time label of LCS.py:158 per window (its last time going forward, its first going backward) and dims
        ``(*lead, timedim, latitude, longitude)``, ``lead`` mapping the dims in front to their coordinates."""
        lat, lon = rec.lat, rec.lon
        if crop and isinstance(self.subdomain, dict):
            mlat, mlon = _crop_strict(lat, lon, self.subdomain)
            a, lat, lon = a[..., mlat, :][..., mlon], lat[mlat], lon[mlon]
        first = np.arange(rec.n_windows) * rec.wstep
        labels = rec.time[first + rec.wlen - 1] if forward else rec.time[first]
        lead = lead or {}
        return _make(rec.like, a, (*lead, self.timedim, "latitude", "longitude"),
                     {**lead, self.timedim: np.asarray(labels), "latitude": lat, "longitude": lon}, name)

    def _departure_out(self, rec: _Record, a, backward):
        """``__call__``'s form of ``x_dep`` / ``y_dep``: ``(latitude, longitude)`` with a scalar time, the last entry of the
        (backward: reversed) time list (LCS.py:161-168 through trajectory.py:141-142)."""
        return _make(rec.like, a, ("latitude", "longitude"),
                     {"latitude": rec.lat, "longitude": rec.lon, self.timedim: rec.time.tolist()[0 if backward else -1]})

    def strain(self, ds=None, u=None, v=None, window=None, stride=1, verbose=True, s=None, resample=None, s_is_error=False,
               isglobal=False, interp_to_common_grid=True, traj_interp_order=3, truncation=20):
        """Both stretch factors of the flow map and its stretching direction: ``(s1, s2, direction)``.

        ``s1 >= s2`` are the singular values of the 3 x 2 Jacobian ``[[dXdx, dXdy], [dYdx, dYdy], [dZdx, dZdy]]`` of
        :func:`flowmap_gradient` -- the PHYSICAL layout, so ``s1`` is not ``__call__``'s value, which takes the 2-norm of the
        reference's row-major 3 x 3 reshape (LCS.py:152-153) --, dims ``(timedim, latitude, longitude)``; ``s1 * s2`` is the
        Lagrangian area change.  ``direction`` has dims ``("component", timedim, latitude, longitude)`` with ``component =
        ["east", "north"]``: the unit vector at the seed that the flow map stretches by ``s1`` (the leading right singular
        vector), signed so that east > 0, or east == 0 and north > 0; ``(1, 0)`` where the cell is isotropic.  A NaN departure
        point gives NaN in all three on the cells whose stencil touches it.

        ``window=None``: one entry, the whole record as ``__call__`` takes it; ``window=k``: the sliding windows of
        :meth:`series` (same ``stride``, same time labels: LCS.py:158 per window).  Intake, ``resample``, sort, regrid / T20
        (:meth:`_record_intake`) and the one pack are shared with :meth:`series`; the direction of integration is the sign of
        ``timestep``.  Then one ``lc_advect_series`` call and one ``lc_strain`` call per memory group (``Engine.lcs_strain``).
        With ``return_dpts`` ``x_dep`` and ``y_dep`` are appended, dims ``(timedim, latitude, longitude)``, as :meth:`series`
        appends them."""
        verboseprint = print if verbose else (lambda *a, **k: None)
        rec = self._record_intake(ds, u, v, window, stride, resample, isglobal, interp_to_common_grid, truncation, verbose)
        verboseprint(f"*---- Parcel propagation: {rec.n_windows} window(s) ----*")
        res = self._run_windows("lcs_strain", rec, rec.timestep, traj_interp_order)
        verboseprint("*---- Done stretch factors ----*")

        forward = np.sign(rec.timestep) == 1
        e = np.stack([_to_np(res["e_lon"]), _to_np(res["e_lat"])])
        out = (self._windows_out(rec, forward, _to_np(res["s1"]), "s1"), self._windows_out(rec, forward, _to_np(res["s2"]), "s2"),
               self._windows_out(rec, forward, e, "direction", lead={"component": np.array(["east", "north"])}))
        if self.return_dpts:                                               # LCS.py:161-168
            out += (self._windows_out(rec, forward, _to_np(res["x_dep"]), crop=False),
                    self._windows_out(rec, forward, _to_np(res["y_dep"]), crop=False))
        return out

    def fsle(self, ds=None, u=None, v=None, ratio=None, final_separation=None, window=None, stride=1, verbose=True, s=None,
             resample=None, s_is_error=False, isglobal=False, interp_to_common_grid=True, traj_interp_order=3, truncation=20,
             level_chunk=16):
        """Finite-size Lyapunov exponents: ``(fsle, tau)``, both with dims ``("threshold", timedim, latitude, longitude)``.

        ``tau`` is the time (seconds, positive) the first of a cell's neighbour pairs -- east, west, north, south on the
        output grid; across the ±180 seam with ``isglobal`` -- takes to separate from its initial great-circle distance ``d0``
        to the threshold ``T``, linearly interpolated between the two time levels that bracket the crossing, and ``fsle =
        ln(T / d0) / tau`` (1/s); both NaN where no pair reaches ``T`` inside the window.  Exactly one of ``ratio`` (``T =
        ratio * d0``, each ``> 1``) and ``final_separation`` (``T`` in metres, each ``> 0``) is given, a scalar or a sequence of up
        to 8 values: the ``threshold`` coordinate.  Unlike FTLE the exponent does not saturate with the window's length and picks
        out one scale of separation.  The direction of integration is the sign of ``timestep``: a backward run gives the
        attracting field.  The full definition: INTEGRATION.md "Finite-size Lyapunov exponents".

        ``window`` / ``stride``, the intake (``resample``, sort, regrid / T20: :meth:`_record_intake`), the one pack, the
        ``subdomain`` crop and the time labels are :meth:`strain`'s; the windows are a plain loop over ``Engine.fsle``, which
        streams each window's trajectories through ``lc_fsle_update`` in blocks of ``level_chunk`` steps.  With ``return_dpts``
        ``x_dep`` and ``y_dep`` are appended, dims ``(timedim, latitude, longitude)``.  Not with ``aux_grid`` for now."""
        if (ratio is None) == (final_separation is None):
            raise ValueError("fsle: give exactly one of ratio and final_separation")
        if self.aux_grid is not None:
            raise ValueError("fsle: the exponent of the auxiliary parcels is not implemented; use an LCS without aux_grid")
        mode, given = ("ratio", ratio) if ratio is not None else ("distance", final_separation)
        if not self.timestep:
            raise ValueError(f"timestep {self.timestep!r}: fsle needs a non-zero step")
        thr, mode, _, radius = Engine.checked_fsle_options(given, mode, self.timestep, self.earth_r)
        verboseprint = print if verbose else (lambda *a, **k: None)
        rec = self._record_intake(ds, u, v, window, stride, resample, isglobal, interp_to_common_grid, truncation, verbose)
        verboseprint(f"*---- Parcel propagation: {rec.n_windows} window(s) ----*")
        eng = get_engine()
        field, lat_t, lon_t = self._packed_record(eng, rec, traj_interp_order)
        res = [eng.fsle(field, lat_t, lon_t, rec.timestep, thr, mode, t0=w * rec.wstep, nsteps=rec.wlen - 1, level_chunk=level_chunk,
                        SETTLS_order=self.SETTLS_order, interp_order=traj_interp_order, cyclic_xboundary=rec.cyclic_xboundary,
                        radius=radius) for w in range(rec.n_windows)]
        verboseprint("*---- Done finite-size exponents ----*")

        forward = np.sign(rec.timestep) == 1
        lead = {"threshold": thr}
        stack = lambda k, axis: np.stack([_to_np(r[k]) for r in res], axis=axis)
        out = (self._windows_out(rec, forward, stack("fsle", 1), "fsle", lead=lead),
               self._windows_out(rec, forward, stack("tau", 1), "tau", lead=lead))
        if self.return_dpts:                                               # LCS.py:161-168
            out += (self._windows_out(rec, forward, stack("x_dep", 0), crop=False),
                    self._windows_out(rec, forward, stack("y_dep", 0), crop=False))
        return out

    def lavd(self, ds=None, u=None, v=None, window=None, stride=1, deviation="domain", verbose=True, s=None, resample=None,
             s_is_error=False, isglobal=False, interp_to_common_grid=True, traj_interp_order=3, truncation=20, level_chunk=16):
        """Elliptic coherence: ``(lavd, rotation, path_length)``, each with dims ``(timedim, latitude, longitude)``.

        ``lavd`` is the Lagrangian-averaged vorticity deviation of Haller et al. (2016) before the division by time: the
        integral along each parcel's trajectory of ``|omega - mean|`` (trapezoid rule over the time levels; dimensionless),
        ``omega`` the relative vorticity of the wind the parcels see -- the record after ``resample``, sort, regrid and T20
        -- and ``mean`` its area-weighted domain mean at each level.  Coherent vortices are its local maxima.  ``rotation`` is
        the signed integral of ``omega - mean``: positive for counter-clockwise rotation (cyclones in the northern hemisphere).
        ``path_length`` is the great-circle length of the trajectory in metres (the arc-length Lagrangian descriptor).  The
        attrs carry ``integration_time = (window length - 1) |timestep|`` seconds: divide by it for the averages.

        ``deviation``: ``'domain'`` (above), ``'none'`` (integrate ``|omega|`` itself: regional boxes, whose mean means little)
        or one value per time level of the record to subtract.  ``window`` / ``stride``, the intake (:meth:`_record_intake`),
        the one pack, the ``subdomain`` crop and the time labels are :meth:`strain`'s and :meth:`fsle`'s; the vorticity is computed
        and packed once for all windows (``Engine.vorticity``, ``Engine.prepare_tracer``) and each window is streamed through
        ``Engine.lavd`` in blocks of ``level_chunk`` steps.  The direction of integration is the sign of ``timestep``.  With
        ``return_dpts`` ``x_dep`` and ``y_dep`` are appended.  Not with ``aux_grid``.  The full definition: INTEGRATION.md
        "Vortices: LAVD, rotation and path length"."""
        if self.aux_grid is not None:
            raise ValueError("lavd: the integrals of the auxiliary parcels are not implemented; use an LCS without aux_grid")
        if not self.timestep or not np.isfinite(self.timestep):
            raise ValueError(f"timestep {self.timestep!r}: lavd needs a non-zero finite step")
        if isinstance(level_chunk, bool) or int(level_chunk) != level_chunk or int(level_chunk) < 1:
            raise ValueError(f"lavd: level_chunk {level_chunk!r} (at least 1)")
        given = Engine.checked_deviation(deviation)[1]
        if given is not None and not isinstance(resample, str) and not isinstance(ds, str):
            like = ds.u if ds is not None else u                            # the record as given: its levels are the windows' levels
            if like is not None and given.size != np.asarray(like[self.timedim].values).size:
                raise ValueError(f"lavd: {given.size} deviation values for {np.asarray(like[self.timedim].values).size} time levels")
        verboseprint = print if verbose else (lambda *a, **k: None)
        rec = self._record_intake(ds, u, v, window, stride, resample, isglobal, interp_to_common_grid, truncation, verbose)
        Engine.checked_vorticity_options(np.shape(rec.uu), np.shape(rec.vv), rec.lat, rec.lon, deviation, self.earth_r)
        verboseprint(f"*---- Vorticity and parcel propagation: {rec.n_windows} window(s) ----*")
        eng = get_engine()
        dtype = common_dtype(rec.uu, rec.vv, rec.lat, rec.lon)
        omega = eng.vorticity(rec.uu, rec.vv, rec.lat, rec.lon, cyclic=rec.cyclic_xboundary, deviation=deviation, radius=self.earth_r,
                              dtype=dtype)["omega"]
        tracer = eng.prepare_tracer(omega, None, rec.lat, rec.lon, traj_interp_order, dtype=dtype)
        field, lat_t, lon_t = self._packed_record(eng, rec, traj_interp_order)
        res = [eng.lavd(field, tracer, lat_t, lon_t, rec.timestep, t0=w * rec.wstep, nsteps=rec.wlen - 1, level_chunk=int(level_chunk),
                        SETTLS_order=self.SETTLS_order, interp_order=traj_interp_order, cyclic_xboundary=rec.cyclic_xboundary,
                        radius=self.earth_r) for w in range(rec.n_windows)]
        verboseprint("*---- Done vorticity deviation ----*")

        forward = np.sign(rec.timestep) == 1
        attrs = {"integration_time": (rec.wlen - 1) * abs(float(rec.timestep))}
        stack = lambda k: np.stack([_to_np(r[k]) for r in res], axis=0)
        out = tuple(_with_attrs(self._windows_out(rec, forward, stack(k), name), attrs)
                    for k, name in (("lavd", "lavd"), ("rotation", "rotation"), ("length", "path_length")))
        if self.return_dpts:                                               # LCS.py:161-168
            out += (self._windows_out(rec, forward, stack("x_dep"), crop=False),
                    self._windows_out(rec, forward, stack("y_dep"), crop=False))
        return out

    def footprint(self, ds=None, u=None, v=None, receptors=None, weights='area', C=None, grid=None, window=None, stride=1, verbose=True,
                  s=None, resample=None, s_is_error=False, isglobal=False, interp_to_common_grid=True, traj_interp_order=3, truncation=20,
                  level_chunk=16):
        """Where the air that arrives at the output points has been: ``(residence, carried)``, each with dims ``(timedim, latitude,
        longitude)`` on the target grid.

        Every other call form writes what happened to a parcel back on the seed grid; this one bins the trajectories themselves.
        ``residence`` is the time the parcels spent over each cell of the target grid (trapezoid rule over the time levels),
        weighted: ``weights='area'`` weights each parcel by the area of its seed cell, ``R^2 cos(lat) dlat dlon`` (m^2 s: the
        footprint does not depend on how finely the receptors are seeded), ``None`` by 1 (seconds), an array on the seed grid
        by the caller's numbers (non-negative; NaN and 0 leave the parcel out).  ``receptors``: a mask on the seed grid -- a
        ridge mask straight from ``find_ridges_spherical_hessian`` or ``filter_ridges``: ``!= 0`` and not NaN counts -- of the
        parcels to follow; None: all of them (those of ``subdomain``, where one is set).  ``C``: a scalar on the wind's grid and
        time levels (the ``C=`` of ``parcel_propagation``); ``carried`` is its mean over the visits to each cell, NaN where there
        were none; None without ``C``.  ``grid=(lat, lon)``: the centres of the target cells, uniform and ascending; default
        the wind's grid after the intake, its columns wrapping where ``isglobal`` and the longitudes close the circle.

        The attrs carry ``integration_time`` (seconds), ``outside_fraction`` (the share of the visits that fell outside the
        target grid) and ``dropped_values`` (visits whose value was not finite).  ``window`` / ``stride``, the intake, the one
        pack and the time labels are :meth:`lavd`'s; the direction of integration is the sign of ``timestep`` (negative: where
        the air came from).  With ``return_dpts`` ``x_dep`` and ``y_dep`` are appended.  Not with ``aux_grid``.  The full
        definition: INTEGRATION.md "Footprints: where the air came from"."""
        if self.aux_grid is not None:
            raise ValueError("footprint: the trajectories of the auxiliary parcels are not binned; use an LCS without aux_grid")
        if not self.timestep or not np.isfinite(self.timestep):
            raise ValueError(f"timestep {self.timestep!r}: footprint needs a non-zero finite step")
        if isinstance(level_chunk, bool) or int(level_chunk) != level_chunk or int(level_chunk) < 1:
            raise ValueError(f"footprint: level_chunk {level_chunk!r} (at least 1)")
        if isinstance(weights, str) and weights != "area":
            raise ValueError(f"footprint: weights {weights!r} ('area', None or an array on the seed grid)")
        if grid is not None:
            if not isinstance(grid, (tuple, list)) or len(grid) != 2:
                raise ValueError("footprint: grid is (lat, lon), the centres of the target cells")
            grid = tuple(np.asarray(getattr(g, "values", g), dtype=np.float64) for g in grid)
            Engine.checked_footprint_grid(grid[0], grid[1], False)
        verboseprint = print if verbose else (lambda *a, **k: None)
        rec = self._record_intake(ds, u, v, window, stride, resample, isglobal, interp_to_common_grid, truncation, verbose)
        glat, glon = grid if grid is not None else (np.asarray(rec.lat, dtype=np.float64), np.asarray(rec.lon, dtype=np.float64))
        mask = self._seed_mask(receptors, rec)
        if isinstance(weights, str):
            w = Engine.seed_cell_areas(rec.lat, rec.lon, self.earth_r)
        elif weights is not None:
            w = np.asarray(getattr(weights, "values", weights), dtype=np.float64)
            if w.shape != mask.shape:
                raise ValueError(f"footprint: weights of shape {w.shape} on a seed grid of {mask.shape}")
        else:
            w = None if mask.all() else np.ones(mask.shape)
        if w is not None:
            w = np.where(mask, w, 0.0)
            Engine.footprint_weights(w, mask.shape)                            # its refusals, before any device work
        eng = get_engine()
        dtype = common_dtype(rec.uu, rec.vv, rec.lat, rec.lon)
        tracer = None
        if C is not None:
            c = self._tracer_on_record(eng, C, rec, resample, isglobal, interp_to_common_grid)
            tracer = eng.prepare_tracer(c, None, rec.lat, rec.lon, traj_interp_order, dtype=dtype)
        verboseprint(f"*---- Parcel propagation and footprints: {rec.n_windows} window(s) ----*")
        field, lat_t, lon_t = self._packed_record(eng, rec, traj_interp_order)
        res = [eng.footprint(field, lat_t, lon_t, rec.timestep, glat, glon, weights=w, tracer=tracer, t0=k * rec.wstep, nsteps=rec.wlen - 1,
                             level_chunk=int(level_chunk), SETTLS_order=self.SETTLS_order, interp_order=traj_interp_order,
                             cyclic_xboundary=rec.cyclic_xboundary) for k in range(rec.n_windows)]
        verboseprint("*---- Done footprints ----*")

        forward = np.sign(rec.timestep) == 1
        stats = np.sum([_to_np(r["acc"]["stats"]) for r in res], axis=0)
        hits = int(sum(int(r["acc"]["hits"].sum()) for r in res))
        attrs = {"integration_time": (rec.wlen - 1) * abs(float(rec.timestep)),
                 "outside_fraction": float(stats[0]) / float(hits + int(stats[0])) if hits + int(stats[0]) else 0.0,
                 "dropped_values": int(stats[1])}
        target = rec._replace(lat=glat, lon=glon)
        stack = lambda k: np.stack([r[k] if isinstance(r[k], np.ndarray) else _to_np(r[k]) for r in res], axis=0)
        residence = _with_attrs(self._windows_out(target, forward, stack("residence" if weights is None else "mass"), "residence", crop=False), attrs)
        carried = None if tracer is None else _with_attrs(self._windows_out(target, forward, stack("mean_value"), getattr(C, "name", None) or "carried",
                                                                            crop=False), attrs)
        out = (residence, carried)
        if self.return_dpts:                                               # LCS.py:161-168
            out += (self._windows_out(rec, forward, stack("x_dep"), crop=False),
                    self._windows_out(rec, forward, stack("y_dep"), crop=False))
        return out

    def _seed_mask(self, receptors, rec: _Record):
        """The parcels :meth:`footprint` follows, as a boolean mask on the whole seed grid: those of ``subdomain`` (strictly
        inside, as the other call forms crop) that ``receptors`` marks -- a labelled ``(latitude, longitude)`` mask on the seed
        grid's coordinates or on a part of them (a cropped result), or a plain array of the whole or the cropped grid's shape;
        ``!= 0`` and not NaN counts."""
        ny, nx = rec.lat.size, rec.lon.size
        mlat, mlon = np.ones(ny, bool), np.ones(nx, bool)
        if isinstance(self.subdomain, dict):
            mlat, mlon = _crop_strict(rec.lat, rec.lon, self.subdomain)
        inside = mlat[:, None] & mlon[None, :]
        if receptors is None:
            return inside
        if hasattr(receptors, "dims"):
            if set(receptors.dims) != {"latitude", "longitude"}:
                raise ValueError(f"footprint: receptors with dims {tuple(receptors.dims)}: a (latitude, longitude) mask (one plane of a series)")
            vals = np.asarray(receptors.transpose("latitude", "longitude").values)
            la, lo = _coord(receptors, "latitude"), _coord(receptors, "longitude")
            i = np.clip(np.searchsorted(rec.lat, la), 0, ny - 1)
            j = np.clip(np.searchsorted(rec.lon, lo), 0, nx - 1)
            if not (np.array_equal(rec.lat[i], la) and np.array_equal(rec.lon[j], lo)):
                raise ValueError("footprint: the receptors' coordinates are not those of the seed grid")
        else:
            vals = np.asarray(receptors)
            if vals.shape == (ny, nx):
                i, j = np.arange(ny), np.arange(nx)
            elif vals.shape == (int(mlat.sum()), int(mlon.sum())):
                i, j = np.nonzero(mlat)[0], np.nonzero(mlon)[0]
            else:
                raise ValueError(f"footprint: receptors of shape {vals.shape} on a seed grid of {(ny, nx)}")
        vals = vals.astype(np.float64)
        full = np.zeros((ny, nx), bool)
        full[np.ix_(i, j)] = (vals != 0) & ~np.isnan(vals)
        return inside & full

    def _tracer_on_record(self, eng, C, rec: _Record, resample, isglobal, interp_to_common_grid):
        """``C`` as ``(time, latitude, longitude)`` values on the record the engine advects on: resampled and sorted as the wind
        was and, where the wind was regridded, regridded (never truncated)."""
        if set(C.dims) != {"latitude", "longitude", self.timedim}:
            raise ValueError(f"footprint: C with dims {tuple(C.dims)}: the wind's dims")
        if isinstance(resample, str):
            C = C.resample({self.timedim: resample}).interpolate('linear') if _is_xarray(C) else _resample_linear(C, self.timedim, resample)
        c, time, lat, lon = _sorted_tll(C, self.timedim)
        if isglobal and interp_to_common_grid:
            from . import preprocess
            c, lat, lon = preprocess.regrid_common_grid(eng, c, lat, lon)
        if not (np.array_equal(time, rec.time) and np.array_equal(lat, rec.lat) and np.array_equal(lon, rec.lon)):
            raise ValueError("footprint: C's coordinates differ from the wind's")
        return c


def _with_attrs(a, attrs):
    """``a`` with ``attrs`` added to its ``attrs`` mapping (a labelled-array class without one is given one)."""
    try:
        a.attrs.update(attrs)
    except AttributeError:
        a.attrs = dict(attrs)
    return a


def _resample_ratio(t_orig, t_new) -> int:
    """Resampled levels per original level: the resampled times must be uniformly spaced and hold every original time at
    index ``i * r`` -- then each original level is a resampled one and a window of the record is a slice of the resampled
    record (linear interpolation between two original levels reads those two only)."""
    t_orig = np.asarray(t_orig).astype("datetime64[ns]")
    t_new = np.asarray(t_new).astype("datetime64[ns]")
    if t_new.size < 2 or t_orig.size < 2:
        raise ValueError("resample: fewer than two time levels")
    d = np.diff(t_new.astype("int64"))
    if not np.all(d == d[0]) or d[0] <= 0:
        raise ValueError("resample: the resampled time spacing is not uniform")
    r, rem = divmod(int((t_orig[1] - t_orig[0]).astype("int64")), int(d[0]))
    if rem or r < 1 or t_new.size != (t_orig.size - 1) * r + 1 or not np.array_equal(t_new[::r], t_orig):
        raise ValueError("resample: the original levels are not every r-th level of a uniform resampled axis "
                         "(the record's own spacing is not uniform, or the resampling frequency does not divide it)")
    return r
