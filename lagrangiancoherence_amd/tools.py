"""Hot-path helpers of the reference's ``LCS/tools.py`` on the HIP engine.

* ``xr_map_coordinates``           LCS/tools.py:11-48   (one interpolation pass)
* ``derivative_spherical_coords``  LCS/tools.py:248-267
* ``fourth_order_derivative``      LCS/tools.py:190-245 (plain arrays in the reference)

* ``find_ridges_spherical_hessian`` LCS/tools.py:52-155 (the consumer of the FTLE field)
* ``filter_ridges``                 the filter LCS/area_of_influence.py:210-242 passes every raw mask through (imported there
                                    from a package outside the reference: defined here, see its docstring)
* ``distance_to_ridges``            LCS/area_of_influence.py:230-244: ``distance_transform_edt(~ridges_bool)``, of which the
                                    driver keeps ``dist < 12`` as the swath a ridge influences
* ``skeletonize_ridges``            LCS/area_of_influence.py:207: ``skeletonize(ridges.values)``, the thinning between the Hessian
                                    mask and the filter (scikit-image there: the rule is defined here, see its docstring)
* ``dilate_ridges``                 LCS/area_of_influence.py:233: ``binary_dilation(ridges.values)``
* ``threshold_local``               LCS/area_of_influence.py:194-199: ``threshold_local(ftle_local.values, block_size=301,
                                    offset=-.8)`` (scikit-image there: the Gaussian rule it documents is restated here), and
                                    ``above_local_threshold``, that threshold and the driver's comparison with it in one call
* ``track_ridges``                  the filter of LCS/area_of_influence.py:210-211 extended through time: space-time labels of a
                                    ridge series (which ridge is the same ridge as in the plane before, how long it lasts), and
                                    ``persistent_ridges``, the ridges that last at least so many planes (defined here)
* ``ridge_properties``              the per-ridge table behind the filter, on the sphere (``metric='sphere'``: square metres, metres,
                                    centroid and orientation in degrees, area-weighted intensities) or in index units; with
                                    ``labelled=True`` of any label map: the areas of influence ``distance_to_ridges`` hands out --
                                    whose per-zone totals are the driver's last step, LCS/area_of_influence.py's
                                    ``np.sum(ridges_ * pr_)`` -- or the ids of ``track_ridges``.  ``filter_ridges(metric='sphere')``
                                    decides on the same numbers (defined here)
* ``ridge_lines``                   the ridges of a thinned mask as curves: the ordered latitude / longitude points of every line,
                                    its great-circle length, its ends and branch points, the intensity along it -- the vector form
                                    of what ``skeletonize_ridges`` returns, which the reference's chain of rasters never reaches
                                    (defined here)
* ``ridge_transects``                what other fields do beside a ridge: great-circle transects across the traced lines, the
                                    profile of rain, water vapour or pressure against the signed distance from the ridge and its
                                    composite per line -- the well-defined part of ``find_area`` (LCS/area_of_influence.py:17-87;
                                    defined here)
* ``Inverse_weighted_interpolation`` LCS/tools.py:285-299 and its labelled wrapper ``xr_idx_interp`` (LCS/tools.py:302-333): values
                                    known at scattered longitude / latitude points -- what ``parcel_propagation(..., C=)`` samples
                                    along trajectories, at the positions ``return_traj`` hands out -- gridded by inverse-distance
                                    weighting with great-circle distances, the way back to the rasters the rest of the chain takes.
                                    The reference's function is broken as written (``arctan`` for ``arctan2``, NaN where a source
                                    lies on a node): the definition is restated here, see their docstrings

The remaining functions of that module (harvesine, latlonsel) have no caller on the path.
"""
from __future__ import annotations

import numpy as np

from .dropin import _coord, _make, _to_np, get_engine
from .engine import Engine, common_dtype

__all__ = ["xr_map_coordinates", "fourth_order_derivative", "derivative_spherical_coords",
           "find_ridges_spherical_hessian", "filter_ridges", "distance_to_ridges", "skeletonize_ridges", "dilate_ridges",
           "threshold_local", "above_local_threshold", "track_ridges", "persistent_ridges", "ridge_properties", "ridge_lines",
           "ridge_transects", "relative_vorticity", "trajectory_density",
           "Inverse_weighted_interpolation", "xr_idx_interp"]


def xr_map_coordinates(da, new_x, new_y, isglobal=True, order=1):
    """Interpolate a 2-D ``(latitude, longitude)`` field at positions ``new_x, new_y``
    (degrees, shaped like the field).  Signature of LCS/tools.py:11.

    ``isglobal=False`` is unreachable from the hot path and broken in the reference
    (undefined name at tools.py:47); it raises here.
    """
    if not isglobal:
        raise NotImplementedError("isglobal=False references an undefined name in the reference (LCS/tools.py:42-47)")
    f = np.asarray(da.transpose("latitude", "longitude").values)
    lat, lon = _coord(da, "latitude"), _coord(da, "longitude")
    px = np.asarray(getattr(new_x, "values", new_x))
    py = np.asarray(getattr(new_y, "values", new_y))
    eng = get_engine()
    field = eng.prepare_field(f[None], f[None], lat, lon, order, dtype=common_dtype(f, lat, lon, px, py))
    out, _ = eng.sample(field, px, py, level=0, interp_order=order)
    return _make(da, _to_np(out).astype(f.dtype, copy=False), ("latitude", "longitude"),
                 {"latitude": lat, "longitude": lon}, getattr(da, "name", None))


def fourth_order_derivative(arr, dim=0, isglobal=True):
    """4th-order 5-point difference in index space on a 2-D array, result in ``arr.dtype``.
    Signature of LCS/tools.py:191 (numba in the reference)."""
    eng = get_engine()
    a = np.ascontiguousarray(arr)
    return _to_np(eng.index_derivative(a, dim, isglobal))


def derivative_spherical_coords(da, dim=0, isglobal=True):
    """``fourth_order_derivative(values.astype('float32'))`` divided by the metric dx / dy.
    Signature of LCS/tools.py:248."""
    if dim not in (0, 1):
        raise ValueError('Dim must be either 0 or 1.')
    lat, lon = _coord(da, "latitude"), _coord(da, "longitude")
    ilat, ilon = np.argsort(lat, kind="stable"), np.argsort(lon, kind="stable")
    vals = np.asarray(da.transpose("latitude", "longitude").values)[ilat][:, ilon]
    lat, lon = lat[ilat], lon[ilon]
    EARTH_RADIUS = 6371000
    y = lat * np.pi / 180
    dx = (np.pi / 180) * (lon[1] - lon[0]) * EARTH_RADIUS * np.cos(y)
    dy = (np.pi / 180) * (lat[1] - lat[0]) * EARTH_RADIUS
    deriv = fourth_order_derivative(vals.astype('float32'), dim=dim, isglobal=isglobal)
    deriv = deriv / dy if dim == 0 else deriv / dx[:, None]
    return _make(da, deriv, ("latitude", "longitude"), {"latitude": lat, "longitude": lon}, getattr(da, "name", None))


def _hessian_ridges_plane(eng, a, lat, lon, sigma, tolerance_threshold, isglobal):
    """The device side of the 2-D ``find_ridges_spherical_hessian``: ``a`` a float64 ``(latitude, longitude)`` device tensor,
    ``lat`` / ``lon`` ascending.  Returns the device tensors ``(mask, eigmin, dt, vec, ddadx, ddady)``."""
    torch = eng.torch
    if isinstance(sigma, (float, int)) and sigma > 1e-15:                              # tools.py:74-75
        a = eng.gaussian_filter(a, sigma)
    y = lat * np.pi / 180
    dx = eng.to_device((np.pi / 180) * (lon[1] - lon[0]) * 6371000 * np.cos(y), np.float64)[:, None]   # tools.py:255
    dy = (np.pi / 180) * (lat[1] - lat[0]) * 6371000                                   # tools.py:256

    def D(f, dim):   # derivative_spherical_coords: float32 cast, index stencil, metric (tools.py:258-264)
        d = eng.index_derivative(f.to(torch.float32), dim, isglobal).to(torch.float64)   # isglobal: tools.py:77-81
        return d / dy if dim == 0 else d / dx
    ddadx, ddady = D(a, 1), D(a, 0)                                                    # tools.py:77-78
    d2x2, d2y2, dxdy = D(ddadx, 1), D(ddady, 0), D(ddadx, 0)                           # tools.py:79-81
    mask, eigmin, dt, vec = eng.ridge_classify(d2x2, dxdy, d2y2, ddadx, ddady, tolerance_threshold,
                                               return_eigvec=True)
    return mask, eigmin, dt, vec, ddadx, ddady


def _angle_and_masked(torch, vec, eigmin):
    """``angle`` (tools.py:125, of the unmasked vector) and the vector zeroed where ``eigmin >= 0`` (tools.py:133); the
    component axis of ``vec`` is the third from the end, in front of ``(latitude, longitude)``."""
    angle = (180 / np.pi) * torch.atan(vec.select(-3, 0) / vec.select(-3, 1))
    return angle, torch.where((eigmin < 0).unsqueeze(-3), vec, torch.zeros_like(vec))


def find_ridges_spherical_hessian(da, sigma=.5, scheme='first_order', tolerance_threshold=0.0005e-3,
                                  return_eigvectors=False, isglobal=True):
    """Hessian ridge filter in spherical coordinates.  Signature of LCS/tools.py:52-54.

    Returns ``(ridges, eigmin)`` with the input's dimension order: ``ridges`` is 1 where the reference's
    gradient/eigenvector product is within ``tolerance_threshold`` and the Hessian eigenvalue of largest
    magnitude is negative, else 0.  Gaussian smoothing, the five float32-cast 4th-order derivatives and
    the per-point ``numpy.linalg.eig`` (a Python loop in the reference) all run on the device.
    ``isglobal=False``: the longitude stencil is one-sided on the two first / last columns instead of cyclic
    (tools.py:229-244); latitude is the same either way.

    ``return_eigvectors=True`` returns the reference's six-tuple (tools.py:140-147):
    ``(ridges, eigmin, raw product, eigvectors, gradient, angle)`` -- ``eigvectors`` has a leading
    ``eigvectors`` dimension labelled ``['d2dadxdy', 'd2dadydx']`` (the reference builds it from those two
    Hessian planes, tools.py:123-124) and is zeroed where ``eigmin >= 0`` (tools.py:133); ``gradient`` has a
    leading ``elements`` dimension ``['ddadx', 'ddady']``; ``angle`` is ``180/pi * arctan(e0/e1)`` of the
    unmasked vector (tools.py:125).

    An input with more dimensions than ``latitude`` and ``longitude`` (the ``(time, latitude, longitude)`` record of
    ``LCS.series``, ``LCS.bidirectional`` or ``LCS.strain``) is a stack of independent planes: every plane is smoothed and
    differenced on its own -- never across time -- and equals the 2-D call on that plane bit for bit, all of them in the same
    three kernel launches (``Engine.ridges_batch``).  That is this function's definition, not the reference's: its
    ``gaussian_filter(da)`` would smooth a 3-D array across time and then fail at its reshape (tools.py:87-90).  The results
    have the input's dimension order and coordinates, the ``eigvectors`` / ``elements`` dimension leading as above.
    """
    dims = tuple(da.dims)
    lead = tuple(d for d in dims if d not in ("latitude", "longitude"))
    lat, lon = _coord(da, "latitude"), _coord(da, "longitude")
    ilat, ilon = np.argsort(lat, kind="stable"), np.argsort(lon, kind="stable")       # tools.py:70-71
    eng = get_engine()
    torch = eng.torch
    name = getattr(da, "name", None)
    if not lead:
        vals = np.asarray(da.transpose("latitude", "longitude").values, dtype=np.float64)[ilat][:, ilon]
        lat, lon = lat[ilat], lon[ilon]
        mask, eigmin, dt, vec, ddadx, ddady = _hessian_ridges_plane(eng, eng.to_device(vals, np.float64), lat, lon, sigma,
                                                                    tolerance_threshold, isglobal)
        grad = torch.stack([ddadx, ddady]) if return_eigvectors else None
        order, coords = ("latitude", "longitude"), {"latitude": lat, "longitude": lon}
        plain = lambda t: t
        labelled = lambda t: t
    else:
        order = (*lead, "latitude", "longitude")
        vals = np.asarray(da.transpose(*order).values, dtype=np.float64)[..., ilat, :][..., ilon]
        lat, lon = lat[ilat], lon[ilon]
        lead_shape, (ny, nx) = vals.shape[:-2], vals.shape[-2:]
        smooth = isinstance(sigma, (float, int)) and sigma > 1e-15                     # tools.py:74-75
        want = ("mask", "eigmin", "dt", "eigvec", "grad") if return_eigvectors else ("mask", "eigmin")
        res = eng.ridges_batch(np.ascontiguousarray(vals.reshape((-1, ny, nx))), lat, lon, sigma=sigma if smooth else None,
                               tolerance=tolerance_threshold, isglobal=isglobal, want=want)
        mask, eigmin, dt, vec, grad = (res.get(k) for k in ("mask", "eigmin", "dt", "eigvec", "grad"))
        coords = {"latitude": lat, "longitude": lon, **{d: _coord(da, d) for d in lead}}
        plain = lambda t: t.reshape(*lead_shape, ny, nx)                               # (n, ny, nx) -> the lead dimensions
        labelled = lambda t: t.movedim(-3, 0).reshape(2, *lead_shape, ny, nx)          # (n, 2, ny, nx) -> 2 in front

    def out(t, first=None, labels=None):
        if first is None:
            return _make(da, _to_np(plain(t)), order, dict(coords), name).transpose(*dims)       # tools.py:150
        o = _make(da, _to_np(labelled(t)), (first, *order), {**coords, first: np.asarray(labels)}, name)
        return o.transpose(first, *dims)                                               # tools.py:141-147
    if not return_eigvectors:
        return out(mask), out(eigmin)
    angle, vec_masked = _angle_and_masked(torch, vec, eigmin)
    return (out(mask), out(eigmin), out(dt), out(vec_masked, "eigvectors", ["d2dadxdy", "d2dadydx"]),
            out(grad, "elements", ["ddadx", "ddady"]), out(angle))


def filter_ridges(ridges, ftle, criteria, thresholds, verbose=True, connectivity=2, cyclic=False, fill=0.0, metric='index',
                  radius=6371000.0):
    """Keep the connected components of ``ridges`` whose properties, measured on ``ftle``, reach the thresholds.
    The call LCS/area_of_influence.py:210-211 makes: ``filter_ridges(ridges, ftle, criteria=['mean_intensity',
    'major_axis_length'], thresholds=[1.2, 30])``.

    ``ridges`` and ``ftle`` are labelled arrays over the same ``latitude`` and ``longitude`` (sorted ascending here, as
    ``find_ridges_spherical_hessian`` sorts), 2-D, or 3-D with one more dimension (time, member): every plane is then filtered
    on its own, all of them in the same kernel launches.  A pixel is part of a ridge when it is ``!= 0`` and not NaN;
    components are joined over edges (``connectivity=1``) or edges and corners (``2``), and with ``cyclic`` across the seam
    of a global longitude axis.  ``criteria``: names out of ``area``, ``mean_intensity``, ``max_intensity``,
    ``min_intensity``, ``major_axis_length``, ``minor_axis_length`` (index units; ``Engine.component_props`` states the
    formulas); a component is kept when every property is ``>=`` its threshold, a NaN property fails.  Pixels of dropped
    components and the background become ``fill``: ``fill=np.nan`` is the form the driver's next line expects
    (``ridges.where(~isnan(ridges), 0)``).  ``verbose`` is accepted for the driver's signature.

    ``metric='index'`` (the default) is the driver's: its ``30`` is 30 pixels, about 830 km at the equator of a 0.25 degree
    grid and about 415 km at 60 degrees; ``area`` counts pixels whose true size shrinks with ``cos(latitude)`` and
    ``mean_intensity`` weights a polar pixel like an equatorial one.  ``metric='sphere'`` measures the same criteria names on
    the array's own ``latitude`` and ``longitude`` (degrees, distinct, ``|latitude| <= 90``; ``cyclic`` also makes the first
    and last longitude cells share the gap that closes the axis): ``area`` in ``radius^2`` (square metres on the default
    Earth), the axis lengths in the unit of ``radius`` -- the driver's ``30`` becomes ``830e3`` --, ``mean_intensity``
    weighted by cell area; ``max_intensity`` and ``min_intensity`` are the same in both.  ``Engine.component_sphere_props``
    states every formula.  The lengths measure chords, so they saturate for ridges that are not small against the sphere;
    the sums behind ``area``, the lengths and the mean are float64 atomic adds whose last bits can differ from run to run
    (as those of the index metric's mean do), so a threshold should not sit within rounding of a ridge's value.

    Returns the filtered mask in the caller's class and dimension order, in ``ridges``' dtype (float64 unless float32)."""
    if metric not in Engine.METRICS:
        raise ValueError(f"metric {metric!r}: 'index' or 'sphere'")
    for k in criteria:
        if k not in Engine.COMPONENT_PROPS:
            raise ValueError(f"criterion {k!r}: one of {', '.join(Engine.COMPONENT_PROPS)}")
    dims = tuple(ridges.dims)
    lead = [d for d in dims if d not in ("latitude", "longitude")]
    if len(lead) > 1 or len(dims) - len(lead) != 2:
        raise ValueError("ridges: dims (latitude, longitude) and at most one more")
    if set(ftle.dims) != set(dims):
        raise ValueError("ridges and ftle differ in their dims")
    order = (*lead, "latitude", "longitude")
    lat, lon = _coord(ridges, "latitude"), _coord(ridges, "longitude")
    if not (np.array_equal(_coord(ftle, "latitude"), lat) and np.array_equal(_coord(ftle, "longitude"), lon)):
        raise ValueError("ridges and ftle differ in their coordinates")
    ilat, ilon = np.argsort(lat, kind="stable"), np.argsort(lon, kind="stable")
    if metric == 'sphere':
        _check_sphere_grid(lat[ilat], lon[ilon], cyclic, radius)

    def sorted_values(da):
        v = np.asarray(da.transpose(*order).values)
        v = v if v.dtype in (np.float32, np.float64) else v.astype(np.float64)
        return np.ascontiguousarray(v[..., ilat, :][..., ilon])
    eng = get_engine()
    if metric == 'sphere':
        out = eng.filter_components(sorted_values(ridges), sorted_values(ftle), criteria, thresholds, connectivity=connectivity,
                                    cyclic=cyclic, fill=fill, metric=metric, lat=lat[ilat], lon=lon[ilon], radius=radius)
    else:
        out = eng.filter_components(sorted_values(ridges), sorted_values(ftle), criteria, thresholds, connectivity=connectivity,
                                    cyclic=cyclic, fill=fill)
    coords = {"latitude": lat[ilat], "longitude": lon[ilon]}
    if lead:
        coords[lead[0]] = _coord(ridges, lead[0])
    return _make(ridges, _to_np(out), order, coords, getattr(ridges, "name", None)).transpose(*dims)


def _check_sphere_grid(lat, lon, cyclic, radius):
    """Every refusal of the sphere metric's coordinates and radius (``ValueError``), on the host: no engine is needed."""
    Engine.sphere_tables(lat, lon, radius)
    Engine.sphere_cell_tables(lat, lon, cyclic)


def ridge_properties(ridges, intensity=None, connectivity=2, cyclic=False, metric='sphere', radius=6371000.0, labelled=False):
    """The table of the ridges of a mask: where each one is, how large, how long, how it is oriented and how intense --
    what ``filter_ridges`` measures to make its yes / no decision, handed out.  Returns ``(labels, table)``.

    ``ridges`` is a labelled array over ``latitude`` and ``longitude`` (sorted ascending here, as ``filter_ridges`` sorts),
    2-D, or 3-D with one more dimension (time, member): every plane is then measured on its own, all of them in the same
    kernel launches.  ``labelled=False``: ``ridges`` is a mask; a pixel is part of a ridge when it is ``!= 0`` and not NaN,
    and the ridges of each plane are its connected components (``Engine.label_components``: ``connectivity`` 1 edges, 2 edges
    and corners; ``cyclic``: across the longitude seam too), numbered ``1..N`` in the order of their first pixel.
    ``labelled=True``: ``ridges`` already holds labels -- the owner map of ``distance_to_ridges(return_labels=True)``, whose
    areas of influence with a rain field as ``intensity`` give the driver's per-zone totals (``np.sum(ridges_ * pr_)``), or
    the ids of ``track_ridges``.  Positive whole numbers up to ``2^31 - 1`` are labels; 0, negative values and NaN are
    background; a positive non-integer raises ``ValueError``; a label need not be connected.  Every plane is measured on its
    own, so track ids give one row per track AND plane: the track's path and intensity through time.

    ``intensity``: a second field over the same dims and coordinates, or None.

    ``labels``: int32, in the caller's class and dimension order.  ``table``: a dict of 1-D numpy arrays of equal length, one
    row per (plane, label) that has at least one pixel, ordered by plane and then by label: ``plane`` (the index along the
    extra dimension, 0 for 2-D input), ``label``, ``area``, ``major_axis_length``, ``minor_axis_length`` and, with an
    ``intensity``, ``mean_intensity``, ``max_intensity``, ``min_intensity``, ``total_intensity`` (a NaN in a ridge makes all
    four NaN).

    ``metric='sphere'`` (the default) measures on the array's own coordinates (degrees, distinct, ``|latitude| <= 90``;
    ``Engine.component_sphere_props`` states every rounding).  Each pixel is the unit vector ``n`` of its node and carries
    the exact area ``w`` of its cell in steradians (band edges at the midpoints between neighbouring coordinates, the outer
    ones half a spacing out and clipped at the poles; with ``cyclic`` the first and last longitude cells share the gap that
    closes the axis).  With ``m`` the ``w``-weighted mean of ``n`` about the ridge's first pixel, ``C`` the weighted
    covariance of ``n`` and ``e1 >= e2 >= e3`` its eigenvalues: ``area`` = ``radius^2 sum w`` (square metres on the default
    Earth); ``major_axis_length`` = ``4 radius sqrt(e1)``, ``minor_axis_length`` = ``4 radius sqrt(e2)`` -- for a ridge that
    is small against the sphere the regionprops formula of the index metric, in the unit of ``radius``; they measure CHORDS
    and so saturate for planet-sized ridges --; ``centroid_latitude``, ``centroid_longitude``: degrees, the direction of the
    weighted mean of ``n`` (NaN where that mean is shorter than ``1e-6``: a ridge spread evenly round the globe has no
    centre); ``orientation``: degrees in ``(-90, 90]``, the angle of the eigenvector of ``e1`` from east towards north at
    the centroid -- 0 zonal, 90 meridional, positive from SW to NE; NaN for a single pixel; ``mean_intensity`` is weighted by
    cell area and ``total_intensity`` = ``radius^2 sum w v``, the area integral of the field over the ridge.  The sums are
    float64 atomic adds whose order is not fixed: the last bits of every float column can differ from run to run.

    ``metric='index'``: ``Engine.component_props``' values in index units, ``centroid_row`` and ``centroid_column`` (of the
    sorted array) instead of the three columns of the sphere, and ``total_intensity`` the plain sum (its last bits, and the
    mean's, can differ from run to run as well)."""
    if metric not in Engine.METRICS:
        raise ValueError(f"metric {metric!r}: 'index' or 'sphere'")
    if connectivity not in (1, 2):
        raise ValueError(f"connectivity {connectivity!r}: 1 (edges) or 2 (edges and corners)")
    dims = tuple(ridges.dims)
    lead = [d for d in dims if d not in ("latitude", "longitude")]
    if len(lead) > 1 or len(dims) - len(lead) != 2:
        raise ValueError("ridges: dims (latitude, longitude) and at most one more")
    order = (*lead, "latitude", "longitude")
    lat, lon = _coord(ridges, "latitude"), _coord(ridges, "longitude")
    if intensity is not None:
        if set(intensity.dims) != set(dims):
            raise ValueError("ridges and intensity differ in their dims")
        if not (np.array_equal(_coord(intensity, "latitude"), lat) and np.array_equal(_coord(intensity, "longitude"), lon)):
            raise ValueError("ridges and intensity differ in their coordinates")
    ilat, ilon = np.argsort(lat, kind="stable"), np.argsort(lon, kind="stable")
    if metric == 'sphere':
        _check_sphere_grid(lat[ilat], lon[ilon], cyclic, radius)

    def sorted_values(da, keep=(np.float32, np.float64)):
        v = np.asarray(da.transpose(*order).values)
        v = v if v.dtype in keep else v.astype(np.float64)
        return np.ascontiguousarray(v[..., ilat, :][..., ilon])
    if labelled:
        v = sorted_values(ridges, keep=(np.float64,))          # every int32 and float32 is a float64
        positive = v > 0                                       # False on NaN
        if (v[positive] != np.floor(v[positive])).any():
            raise ValueError("ridges: with labelled=True every positive value is a whole number (a label)")
        if positive.any() and v[positive].max() > 2 ** 31 - 1:
            raise ValueError("ridges: with labelled=True labels are at most 2^31 - 1")
        host_labels = np.where(positive, v, 0).astype(np.int32)
    else:
        v = sorted_values(ridges)
    w = None if intensity is None else sorted_values(intensity)
    eng = get_engine()
    torch = eng.torch
    if labelled:
        labels = torch.from_numpy(host_labels).to(eng.device).contiguous()
        counts = labels.reshape(1 if labels.dim() == 2 else labels.shape[0], -1).amax(dim=1).to(torch.int32)
    else:
        labels, counts = eng.label_components(eng.to_device(v, v.dtype), connectivity, cyclic)
    if w is not None:
        w = eng.to_device(w, w.dtype)
    if metric == 'sphere':
        props = eng.component_sphere_props(labels, counts, lat[ilat], lon[ilon], w, cyclic, radius)
        names = [k for k in ("area", "major_axis_length", "minor_axis_length", "mean_intensity", "max_intensity", "min_intensity",
                             "total_intensity", "centroid_latitude", "centroid_longitude", "orientation") if k in props]
    else:
        props = eng.component_props(labels, counts, w, cyclic)
        props["centroid_row"], props["centroid_column"] = props["centroid"][..., 0], props["centroid"][..., 1]
        names = ["area", "major_axis_length", "minor_axis_length"]
        if w is not None:
            props["total_intensity"] = torch.where(props["area"] > 0, eng.component_sums(labels, counts, w, cyclic)["sum"].reshape(
                props["area"].shape), torch.full_like(props["mean_intensity"], float("nan")))
            names += ["mean_intensity", "max_intensity", "min_intensity", "total_intensity"]
        names += ["centroid_row", "centroid_column"]
    area = _to_np(props["area"])
    area = area if area.ndim == 2 else area[None]
    plane, index = np.nonzero(area > 0)                        # by plane, then by label
    table = {"plane": plane.astype(np.int64), "label": (index + 1).astype(np.int32)}
    for k in names:
        col = _to_np(props[k])
        table[k] = (col if col.ndim == 2 else col[None])[plane, index]
    coords = {"latitude": lat[ilat], "longitude": lon[ilon]}
    if lead:
        coords[lead[0]] = _coord(ridges, lead[0])
    return _make(ridges, _to_np(labels), order, coords, getattr(ridges, "name", None)).transpose(*dims), table


LINE_COLUMNS = ("plane", "line", "offset", "count", "closed", "first_latitude", "first_longitude", "last_latitude", "last_longitude",
                "first_degree", "last_degree", "length", "chord", "sinuosity", "component")
POINT_COLUMNS = ("line", "latitude", "longitude", "row", "column", "distance")


def ridge_lines(ridges, intensity=None, cyclic=False, metric='sphere', radius=6371000.0):
    """The ridges of a thinned mask as curves: the ordered latitude / longitude points of every line, its arc length, where it
    ends and where it branches, and the intensity along it -- the vector form of what ``skeletonize_ridges`` returns, for
    plotting, export and measuring (``Engine.trace_lines``; include/lcs_hip.h states the definition).  Returns
    ``(lines, points)``, two dicts of numpy arrays.

    ``ridges`` is a labelled array over ``latitude`` and ``longitude`` (sorted ascending here, as ``filter_ridges`` sorts),
    2-D, or 3-D with one more dimension (time, member): every plane is then traced on its own, all of them in the same
    kernel launches.  A pixel is part of a ridge when it is ``!= 0`` and not NaN.  It is linked to its ridge neighbours N, E,
    S, W, and to a diagonal one only where neither pixel beside both is ridge: a staircase is a path.  Pixels with two links
    are interior; all others are nodes (no link: a lone pixel; one: a free end; three or more: a junction).  A line runs
    from node to node through interior pixels, or is a ring of interior pixels.  ``cyclic``: the last longitude is the
    western neighbour of the first (at least 3 longitudes).  The mask should be one pixel wide: on a thick one nearly every
    pixel is a junction and every link a line of two points.

    ``lines`` has one row per line, ordered by plane, then by the line's first link in raster order: ``plane`` (the index
    along the extra dimension, 0 for 2-D input), ``line`` (its number within the plane), ``offset``, ``count`` (its points
    are ``points[...][offset:offset + count]``), ``closed`` (1: a ring, whose first point is not repeated), ``first_latitude``,
    ``first_longitude``, ``last_latitude``, ``last_longitude``, ``first_degree``, ``last_degree`` (links of the end pixels: 1 a
    free end, >= 3 a junction, 0 a lone pixel, 2 a ring), ``length``, ``chord`` (first to last point; 0 for rings and for loops
    through one junction), ``sinuosity`` (``length / chord``, NaN where the chord is 0) and ``component`` (the line's label
    under ``Engine.label_components(connectivity=2, cyclic)``: the ``label`` of ``ridge_properties``).  With an
    ``intensity`` -- a second field over the same dims and coordinates, the FTLE for instance --: ``mean_intensity``,
    ``max_intensity``, ``min_intensity`` over the line's points.

    ``points`` has one row per point, ordered by line and along it: ``line`` (a row of ``lines``), ``latitude``,
    ``longitude``, ``row``, ``column`` (of the sorted array), ``distance`` (along the line from its first point) and, with
    one, ``intensity``.

    ``metric='sphere'`` (the default): lengths are great-circle arcs in the unit of ``radius`` (metres on the default Earth),
    link by link, from the array's own coordinates in degrees (distinct, ``|latitude| <= 90``).  ``metric='index'``: a link
    counts 1 along an edge and ``sqrt(2)`` across a corner."""
    return _traced_ridge_lines(ridges, intensity, cyclic, metric, radius)[:2]


def _traced_ridge_lines(ridges, intensity, cyclic, metric, radius, before_engine=None):
    """``ridge_lines``' two tables and, for ``ridge_transects``, what they were made from: the engine, the device trace, the
    sorted coordinates and the function that brings a field into the traced order.  ``before_engine(lat, lon, shape)`` runs
    after this function's own checks and before an engine is asked for."""
    if metric not in Engine.METRICS:
        raise ValueError(f"metric {metric!r}: 'index' or 'sphere'")
    dims = tuple(ridges.dims)
    lead = [d for d in dims if d not in ("latitude", "longitude")]
    if len(lead) > 1 or len(dims) - len(lead) != 2:
        raise ValueError("ridges: dims (latitude, longitude) and at most one more")
    order = (*lead, "latitude", "longitude")
    lat, lon = _coord(ridges, "latitude"), _coord(ridges, "longitude")
    if intensity is not None:
        if set(intensity.dims) != set(dims):
            raise ValueError("ridges and intensity differ in their dims")
        if not (np.array_equal(_coord(intensity, "latitude"), lat) and np.array_equal(_coord(intensity, "longitude"), lon)):
            raise ValueError("ridges and intensity differ in their coordinates")
    ilat, ilon = np.argsort(lat, kind="stable"), np.argsort(lon, kind="stable")
    lat, lon = lat[ilat], lon[ilon]
    if metric == 'sphere':
        _check_sphere_grid(lat, lon, cyclic, radius)

    def sorted_values(da):
        v = np.asarray(da.transpose(*order).values)
        v = v if v.dtype in (np.float32, np.float64) else v.astype(np.float64)
        return np.ascontiguousarray(v[..., ilat, :][..., ilon])
    v = sorted_values(ridges)
    Engine.checked_line_options(v.shape, cyclic, metric, lat, lon, radius, None)
    w = None if intensity is None else sorted_values(intensity).astype(np.float64).reshape(-1, lat.size, lon.size)
    if before_engine is not None:
        before_engine(lat, lon, v.shape)
    eng = get_engine()
    mask = eng.to_device(v, v.dtype)
    traced = eng.trace_lines(mask, cyclic, metric, lat if metric == 'sphere' else None, lon if metric == 'sphere' else None, radius)
    labels, _ = eng.label_components(mask, 2, cyclic)
    t = {k: _to_np(x) for k, x in traced.items()}
    labels = _to_np(labels).reshape(-1, lat.size * lon.size)
    nx = lon.size
    plane, first, last = t["plane"].astype(np.int64), t["first"].astype(np.int64), t["last"].astype(np.int64)
    starts = np.flatnonzero(np.diff(plane, prepend=-1) != 0)             # the first line of every plane that has one
    number = np.arange(plane.size) - np.repeat(starts, np.diff(np.append(starts, plane.size)))
    if metric == 'sphere':
        cl, sl, cx, sx = Engine.sphere_tables(lat, lon, radius)[:4]

        def unit(p):
            r, c = p // nx, p % nx
            return cl[r] * cx[c], cl[r] * sx[c], sl[r]
        (xa, ya, za), (xb, yb, zb) = unit(first), unit(last)
        dx, dy, dz = xa - xb, ya - yb, za - zb
        chord = 2.0 * float(radius) * np.arcsin(np.minimum(1.0, np.sqrt((dx * dx + dy * dy) + dz * dz) / 2.0))
    else:
        chord = np.hypot((first // nx - last // nx).astype(np.float64), (first % nx - last % nx).astype(np.float64))
    chord = np.where(t["closed"] != 0, 0.0, chord)
    with np.errstate(divide="ignore", invalid="ignore"):
        sinuosity = np.where(chord > 0, t["length"] / chord, np.nan)
    lines = {"plane": plane, "line": number.astype(np.int64), "offset": t["offset"].astype(np.int64), "count": t["count"].astype(np.int64),
             "closed": t["closed"].astype(np.uint8),
             "first_latitude": lat[first // nx], "first_longitude": lon[first % nx],
             "last_latitude": lat[last // nx], "last_longitude": lon[last % nx],
             "first_degree": t["first_degree"].astype(np.int32), "last_degree": t["last_degree"].astype(np.int32),
             "length": t["length"], "chord": chord, "sinuosity": sinuosity,
             "component": labels[plane, first].astype(np.int32)}
    pixel = t["pixel"].astype(np.int64)
    points = {"line": t["line"].astype(np.int64), "latitude": lat[pixel // nx], "longitude": lon[pixel % nx],
              "row": (pixel // nx).astype(np.int32), "column": (pixel % nx).astype(np.int32), "distance": t["distance"]}
    if w is not None:
        value = w.reshape(w.shape[0], -1)[plane[points["line"]], pixel]
        points["intensity"] = value
        # per line: its points are one contiguous run
        at = lines["offset"][lines["count"] > 0]
        for name, op in (("max_intensity", np.maximum), ("min_intensity", np.minimum)):
            lines[name] = op.reduceat(value, at) if at.size else np.zeros(0)
        lines["mean_intensity"] = (np.add.reduceat(value, at) / lines["count"]) if at.size else np.zeros(0)
    return lines, points, {"engine": eng, "trace": traced, "lat": lat, "lon": lon, "sorted_values": sorted_values}


def ridge_transects(ridges, fields, half_width, spacing, smooth=3, orient='left', method='linear', cyclic=False, radius=6371000.0):
    """What other fields do beside a ridge: every field of ``fields`` sampled along great circles across the lines of a
    thinned mask, as a function of the signed distance from the line, and the composite of those profiles per line -- the rain,
    water vapour or pressure profile across a convergence zone, which the reference's driver approximates by painting pixels
    along the Hessian eigenvector (``find_area``, LCS/area_of_influence.py:17-87; its painted mask is not reproduced: it steps in
    degrees, which is wrong away from the equator, and gives the normal's sign no meaning).  Returns ``(lines, points,
    transects)`` (``Engine.ridge_transects``; include/lcs_hip.h states the definition).

    ``ridges``: as for ``ridge_lines`` -- a thinned mask over ``latitude`` and ``longitude`` with at most one more dimension,
    sorted ascending here; a pixel is foreground when it is ``!= 0`` and not NaN.  ``lines`` and ``points`` are exactly what
    ``ridge_lines(ridges, None, cyclic, 'sphere', radius)`` returns; ``points`` additionally carries ``normal_east``,
    ``normal_north`` (the components of the unit normal the transect leaves the point along, towards positive offsets) and
    ``heading`` (degrees clockwise from north of the direction of travel along the line, in ``[0, 360)``; NaN where the point
    has no tangent: lone pixels and lines of one point).

    ``fields``: one labelled array, or a dict of name -> array, each with the dims and coordinates of ``ridges``; float32 or
    float64 (anything else is converted to float64; mixed dtypes to float64), and the results take that dtype.  With a 3-D
    input the points of each plane read that plane of every field.

    The transect through a point is the great circle at right angles to the line there -- to the chord between the points
    ``smooth`` before and after it along the line, clamped at the ends of an open line and wrapped on a ring.  It is sampled at
    the offsets ``s_k = k * spacing`` for ``k = -K .. K``, ``K = floor(half_width / spacing)``, in the unit of ``radius`` (metres
    on the default Earth).  ``orient='left'``: positive offsets lie to the left of the direction of travel; ``'north'``: on the
    side whose normal has a positive north component (east where it has none); ``'east'``: likewise with east first.
    ``method='linear'``: bilinear in degrees between the four nodes around the position, NaN where one of them is NaN;
    ``'nearest'``: the nearer node in each axis.  The latitudes need not be uniform.  Positions outside the grid are NaN;
    ``cyclic``: longitudes are wrapped into ``[longitude[0], longitude[0] + 360)`` and the cell after the last one ends at the
    first (a span below 360 degrees).

    ``transects`` is a dict of numpy arrays with ``M = 2 K + 1``: ``offset`` ``(M,)``; ``latitude``, ``longitude`` ``(n_points,
    M)`` float64, the sample positions in degrees as the device wrote them; ``values`` ``(n_fields, n_points, M)``, or a dict by
    name when a dict was given; ``line_mean`` and ``line_count`` ``(n_fields, n_lines, M)`` (dicts likewise): the mean of the
    finite values over the points of each line, offset by offset, and how many entered it (NaN where none did).  The
    cross-ridge gradient at the ridge is ``(values[:, :, K + 1] - values[:, :, K - 1]) / (2 * spacing)``."""
    named = isinstance(fields, dict)
    group = dict(fields) if named else {None: fields}
    if not group:
        raise ValueError("fields: a labelled array or a dict of name -> array with at least one entry")
    dims = tuple(ridges.dims)
    glat, glon = _coord(ridges, "latitude"), _coord(ridges, "longitude")
    for name, da in group.items():
        if not hasattr(da, "dims") or set(da.dims) != set(dims):
            raise ValueError(f"ridges and fields{'' if name is None else f'[{name!r}]'} differ in their dims")
        if not (np.array_equal(_coord(da, "latitude"), glat) and np.array_equal(_coord(da, "longitude"), glon)):
            raise ValueError(f"ridges and fields{'' if name is None else f'[{name!r}]'} differ in their coordinates")
        if dict(zip(da.dims, np.shape(da.values))) != dict(zip(dims, np.shape(ridges.values))):
            raise ValueError(f"ridges and fields{'' if name is None else f'[{name!r}]'} differ in their shapes")

    def check(lat, lon, shape):                                                # every refusal, before a device
        Engine.checked_transect_options(shape, lat, lon, half_width, spacing, smooth, orient, method, cyclic, radius)
    lines, points, made = _traced_ridge_lines(ridges, None, cyclic, 'sphere', radius, before_engine=check)
    stack = [made["sorted_values"](da) for da in group.values()]
    dtype = stack[0].dtype if all(v.dtype == stack[0].dtype for v in stack) else np.dtype(np.float64)
    stack = np.stack([v.astype(dtype, copy=False) for v in stack])
    got = made["engine"].ridge_transects(made["trace"], stack, made["lat"], made["lon"], half_width, spacing, smooth, orient,
                                         method, cyclic, radius)
    got = {k: _to_np(v) for k, v in got.items()}
    points["normal_east"], points["normal_north"] = got["normal_east"], got["normal_north"]
    with np.errstate(invalid="ignore"):
        heading = np.mod(np.degrees(np.arctan2(got["tangent_east"], got["tangent_north"])), 360.0)
        points["heading"] = np.where(heading >= 360.0, 0.0, heading)        # (a tiny negative angle rounds up to 360 itself)

    def by_name(a):
        return {name: a[k] for k, name in enumerate(group)} if named else a
    transects = {"offset": got["offset"], "latitude": got["latitude"], "longitude": got["longitude"], "values": by_name(got["values"]),
                 "line_mean": by_name(got["line_mean"]), "line_count": by_name(got["line_count"])}
    return lines, points, transects


def distance_to_ridges(ridges, cyclic=False, sampling=None, max_distance=None, return_labels=False, connectivity=2,
                       metric='index', radius=6371000.0):
    """Distance from every grid point to the nearest ridge pixel, on the device.  ``metric='index'`` (the default):
    ``scipy.ndimage.distance_transform_edt(~ridges_bool)`` of LCS/area_of_influence.py:231, bit for bit
    (``Engine.distance_transform``).  ``metric='sphere'``: the great-circle distance on the array's own ``latitude`` and
    ``longitude`` (``Engine.sphere_distance``).

    ``ridges`` is a labelled array over ``latitude`` and ``longitude`` (sorted ascending here, as ``filter_ridges`` sorts),
    2-D, or 3-D with one more dimension (time, member): every plane is then transformed on its own, all of them in the same
    kernel launches.  A pixel is part of a ridge when it is ``!= 0`` and not NaN.  A plane without a ridge is ``+inf``
    everywhere.

    ``metric='index'``: distances are in INDEX units times ``sampling`` (a scalar or ``(latitude step, longitude step)``,
    default 1), as the driver's are.  ``cyclic``: longitude offsets are taken the shorter way round a global axis.
    ``max_distance``: points further away are ``+inf`` and cost no search -- ``max_distance=12`` is the driver's
    ``dist.where(dist < 12)`` up to the points at exactly 12, which it drops and this keeps.

    ``metric='sphere'``: distances are great-circle distances in the unit of ``radius`` (metres on the default Earth), from
    the coordinates in degrees, which need be neither uniform nor global: ``2 radius asin(chord / 2)`` of the smallest chord
    between the unit vectors of the two nodes, float64 (``Engine.sphere_distance`` states every rounding).  On a
    latitude-longitude grid the index metric is wrong by ``1 / cos(latitude)`` along longitude and blind across the poles;
    this one is neither, and it sees across the seam without a flag: ``cyclic`` then applies to the labels only.
    ``max_distance`` is in the unit of ``radius`` -- ``max_distance=330e3`` is the swath within 330 km of a ridge, what the
    driver's ``dist < 12`` stands for at 0.25 degrees -- and cuts the search to the latitudes within it.  ``sampling`` has no
    meaning here and must be None.  Every point is compared with every ridge pixel within the bound's band of latitudes.

    ``return_labels=True`` also returns, per point, the label of the ridge its nearest pixel belongs to (0 where the distance
    is ``+inf``): ``Engine.label_components(ridges, connectivity, cyclic)`` gathered through the nearest-pixel index, on the
    device.  Among equally near pixels the one of smallest (latitude, longitude) index decides.  That is the partition of the
    plane into every ridge's own area of influence, which the driver approximates by dilation and a second filter.

    Returns float64 distances (and int32 labels) in the caller's class and dimension order."""
    if metric not in ('index', 'sphere'):
        raise ValueError(f"metric {metric!r}: 'index' or 'sphere'")
    if metric == 'sphere' and sampling is not None:
        raise ValueError("sampling belongs to metric='index': on the sphere the coordinates are the metric")
    dims = tuple(ridges.dims)
    lead = [d for d in dims if d not in ("latitude", "longitude")]
    if len(lead) > 1 or len(dims) - len(lead) != 2:
        raise ValueError("ridges: dims (latitude, longitude) and at most one more")
    order = (*lead, "latitude", "longitude")
    lat, lon = _coord(ridges, "latitude"), _coord(ridges, "longitude")
    ilat, ilon = np.argsort(lat, kind="stable"), np.argsort(lon, kind="stable")
    if metric == 'sphere':
        Engine.sphere_tables(lat, lon, radius, max_distance)        # every refusal of the coordinates and the bound, before a device
    v = np.asarray(ridges.transpose(*order).values)
    v = v if v.dtype in (np.float32, np.float64) else v.astype(np.float64)
    v = np.ascontiguousarray(v[..., ilat, :][..., ilon])
    eng = get_engine()
    mask = eng.to_device(v, v.dtype)
    coords = {"latitude": lat[ilat], "longitude": lon[ilon]}
    if lead:
        coords[lead[0]] = _coord(ridges, lead[0])

    def out(t):
        return _make(ridges, _to_np(t), order, coords, getattr(ridges, "name", None)).transpose(*dims)

    def transform(return_nearest=False):
        if metric == 'sphere':
            return eng.sphere_distance(mask, lat[ilat], lon[ilon], radius, max_distance, return_nearest=return_nearest)
        return eng.distance_transform(mask, cyclic, sampling, max_distance, return_nearest=return_nearest)
    if not return_labels:
        return out(transform())
    dist, nearest = transform(return_nearest=True)
    labels, _ = eng.label_components(mask, connectivity, cyclic)
    planes = labels.reshape(-1, labels.shape[-2] * labels.shape[-1])
    index = nearest.reshape(planes.shape).to(eng.torch.int64)
    owner = eng.torch.where(index >= 0, planes.gather(1, index.clamp(min=0)), eng.torch.zeros_like(planes))
    return out(dist), out(owner.reshape(labels.shape))


def _ridge_planes(ridges):
    """What the two morphological functions share: ``ridges`` sorted as ``filter_ridges`` sorts it, on the device with the
    extra dimension (if any) leading, and the way back to the caller's class, dimension order and dtype."""
    dims = tuple(ridges.dims)
    lead = [d for d in dims if d not in ("latitude", "longitude")]
    if len(lead) > 1 or len(dims) - len(lead) != 2:
        raise ValueError("ridges: dims (latitude, longitude) and at most one more")
    order = (*lead, "latitude", "longitude")
    lat, lon = _coord(ridges, "latitude"), _coord(ridges, "longitude")
    ilat, ilon = np.argsort(lat, kind="stable"), np.argsort(lon, kind="stable")
    v = np.asarray(ridges.transpose(*order).values)
    dtype = v.dtype
    v = v if dtype in (np.float32, np.float64) else v.astype(np.float64)
    v = np.ascontiguousarray(v[..., ilat, :][..., ilon])
    eng = get_engine()
    coords = {"latitude": lat[ilat], "longitude": lon[ilon]}
    if lead:
        coords[lead[0]] = _coord(ridges, lead[0])

    def out(t):
        return _make(ridges, _to_np(t).astype(dtype, copy=False), order, coords, getattr(ridges, "name", None)).transpose(*dims)
    return eng, eng.to_device(v, v.dtype), out


def skeletonize_ridges(ridges, method='guohall', cyclic=False, max_iterations=None, table=None, fill=0.0):
    """Thin every ridge of a mask to a line one pixel wide, on the device (``Engine.thin``): the step
    ``skeletonize(ridges.values)`` of LCS/area_of_influence.py:207, between ``find_ridges_spherical_hessian`` -- whose mask is
    several pixels wide -- and ``filter_ridges``, whose ``major_axis_length`` is meant for the thinned line.

    ``ridges`` is a labelled array over ``latitude`` and ``longitude`` (sorted ascending here, as ``filter_ridges`` sorts),
    2-D, or 3-D with one more dimension (time, member): every plane is then thinned on its own, all of them in the same
    kernel launches.  A pixel is part of a ridge when it is ``!= 0`` and not NaN; pixels outside the plane are background;
    with ``cyclic`` the last longitude is the western neighbour of the first.

    The rule is a parallel thinning in two sub-iterations, driven by a table of 256 codes indexed by the neighbourhood
    ``NW + 2 N + 4 NE + 8 E + 16 SE + 32 S + 64 SW + 128 W`` (N is row r - 1 of the plane as it is sorted): bit 0 of a code
    deletes the pixel in the first sub-iteration, bit 1 in the second; every sub-iteration reads the whole plane as the one
    before left it; it ends when an iteration deletes nothing, or after ``max_iterations``.  ``method`` names a shipped table
    (``Engine.thinning_table`` states both rules): ``'guohall'`` (Guo & Hall 1989, the default) kept the number of
    8-connected components on every mask it was tried on and leaves one pixel of a 2 x 2 block; ``'zhang'`` (Zhang & Suen
    1984) deletes a 2 x 2 block entirely and so can lose small ridges, which would then silently be missing from
    ``filter_ridges`` too.  ``table`` takes the caller's own 256 codes instead.  scikit-image's own table is NOT reproduced
    here: the package is not a dependency of this project and was not at hand to generate or check it against; a user who
    has it can pass its table (recoded to the two bits above) and get its skeleton.

    Returns the mask in the caller's class, dimension order and dtype: the input's value on the pixels that survive,
    ``fill`` elsewhere."""
    if table is None:
        table = Engine.thinning_table(method)          # ValueError for a method that is not shipped
    table = Engine.checked_thinning_table(table)
    if max_iterations is not None and int(max_iterations) < 1:
        raise ValueError(f"max_iterations {max_iterations!r}: >= 1, or None for no bound")
    eng, mask, out = _ridge_planes(ridges)
    keep = eng.thin(mask, table, cyclic=cyclic, max_iterations=max_iterations)
    return out(eng.torch.where(keep != 0, mask, eng.torch.full_like(mask, float(fill))))


def dilate_ridges(ridges, iterations=1, connectivity=1, cyclic=False, fill=0.0):
    """Grow every ridge of a mask by one pixel per iteration, on the device (``Engine.dilate``): ``binary_dilation(
    ridges.values)`` of LCS/area_of_influence.py:233.  A background pixel becomes part of a ridge when one of its four edge
    neighbours (``connectivity=1``: the default of ``skimage.morphology.binary_dilation``, which the driver uses, and of
    ``scipy.ndimage.binary_dilation``) or of its eight neighbours (``2``) is; ``iterations`` times.

    ``ridges``, foreground, planes and ``cyclic`` as for ``skeletonize_ridges``.  Returns the mask in the caller's class,
    dimension order and dtype: the input's value on the pixels that were ridge already, 1 on the added ones, ``fill``
    elsewhere."""
    if connectivity not in Engine.STRUCTURES:
        raise ValueError(f"connectivity {connectivity!r}: 1 (edges) or 2 (edges and corners)")
    if int(iterations) < 1:
        raise ValueError(f"iterations {iterations!r}: >= 1")
    eng, mask, out = _ridge_planes(ridges)
    torch = eng.torch
    grown = eng.dilate(mask, iterations=iterations, connectivity=connectivity, cyclic=cyclic)
    was = (mask != 0) & ~torch.isnan(mask)
    added = torch.where(grown != 0, torch.ones_like(mask), torch.full_like(mask, float(fill)))
    return out(torch.where(was, mask, added))


def _ridge_record(ridges, connectivity, reach, min_duration):
    """What the two tracking functions share: every argument check, before an engine exists; then ``ridges`` sorted as
    ``filter_ridges`` sorts it, on the device as ``(time, latitude, longitude)``, and the way back to the caller's class and
    dimension order.  Returns ``(engine, record, out, time coordinate, connectivity, reach, min_duration)``."""
    connectivity, reach = Engine.checked_track_options(connectivity, reach)
    if isinstance(min_duration, bool) or not isinstance(min_duration, (int, np.integer)) or min_duration < 1:
        raise ValueError(f"min_duration {min_duration!r}: an integer >= 1 (planes)")
    dims = tuple(ridges.dims)
    lead = [d for d in dims if d not in ("latitude", "longitude")]
    if len(lead) != 1 or len(dims) != 3:
        raise ValueError("ridges: dims latitude, longitude and exactly one more (the time a ridge is followed through)")
    order = (lead[0], "latitude", "longitude")
    lat, lon = _coord(ridges, "latitude"), _coord(ridges, "longitude")
    ilat, ilon = np.argsort(lat, kind="stable"), np.argsort(lon, kind="stable")
    v = np.asarray(ridges.transpose(*order).values)
    dtype = v.dtype
    v = v if dtype in (np.float32, np.float64) else v.astype(np.float64)
    v = np.ascontiguousarray(v[..., ilat, :][..., ilon])
    time = _coord(ridges, lead[0])
    coords = {lead[0]: time, "latitude": lat[ilat], "longitude": lon[ilon]}
    eng = get_engine()

    def out(t, keep_dtype=False):
        a = _to_np(t)
        return _make(ridges, a.astype(dtype, copy=False) if keep_dtype else a, order, coords, getattr(ridges, "name", None)).transpose(*dims)
    return eng, eng.to_device(v, v.dtype), out, time, connectivity, reach, int(min_duration)


def track_ridges(ridges, reach=1, connectivity=2, cyclic=False, min_duration=1, return_table=False):
    """Follow the ridges of a mask series through time, on the device (``Engine.label_tracks``): which ridge of a plane is
    the same ridge as in the plane before, and how long it lasts -- what ``filter_ridges`` (LCS/area_of_influence.py:210-211)
    cannot measure, because its components end at the plane.

    ``ridges`` is a labelled array over ``latitude``, ``longitude`` (sorted ascending here, as ``filter_ridges`` sorts) and
    exactly one more dimension, the time; its planes are taken in the order given, consecutive means adjacent index, nothing
    is sorted along time.  A voxel is part of a ridge when it is ``!= 0`` and not NaN.  Two ridge voxels are linked when they
    are neighbours in one plane (``connectivity`` 1: edges, 2: edges and corners; ``cyclic``: across the longitude seam too),
    or lie in adjacent planes at most ``reach`` pixels apart in both latitude and longitude index (``cyclic``: the longitude
    offset the shorter way round); ``reach`` is an integer in 0 .. 16, 0 meaning the same pixel.  A track is a connected
    component of that relation: ridges that MERGE or SPLIT therefore belong to one track, which is not cut where they meet.
    A thinned ridge moves, so ``reach`` should be about its displacement per time step in pixels (or dilate first).

    Returns int32 track ids in the caller's class and dimension order: 0 off the ridges, else ``1..N`` in the order of each
    track's first voxel in ``(time, latitude, longitude)`` raster order.  Tracks that occupy fewer than ``min_duration``
    consecutive-index planes (``last - first + 1``) become 0 and the survivors are renumbered ``1..M`` in the same order.
    ``return_table=True`` also returns a dict of numpy arrays with one entry per surviving track: ``first``, ``last`` (plane
    indices), ``duration``, ``volume`` (voxels), and ``first_time``, ``last_time``, the time coordinate's labels there."""
    eng, record, out, time, connectivity, reach, min_duration = _ridge_record(ridges, connectivity, reach, min_duration)
    torch = eng.torch
    labels, count = eng.label_tracks(record, connectivity, cyclic, reach)
    spans = eng.track_spans(labels, count)
    keep = (spans["volume"] > 0) & (spans["duration"] >= min_duration)
    # new id of every old one: the running count of the kept tracks, 0 for a dropped one and for the background
    new_id = torch.where(keep, torch.cumsum(keep.to(torch.int32), 0, dtype=torch.int32), torch.zeros_like(spans["first"]))
    table = torch.cat([torch.zeros((1,), dtype=torch.int32, device=new_id.device), new_id])
    ids = table.gather(0, labels.reshape(-1).to(torch.int64)).reshape(labels.shape)
    if not return_table:
        return out(ids)
    kept = {k: _to_np(spans[k][keep]) for k in ("first", "last", "duration", "volume")}
    kept["first_time"], kept["last_time"] = np.asarray(time)[kept["first"]], np.asarray(time)[kept["last"]]
    return out(ids), kept


def persistent_ridges(ridges, min_duration, reach=1, connectivity=2, cyclic=False, fill=0.0):
    """Keep the ridges that last: ``filter_ridges``' convention along time (``Engine.filter_tracks``).  The input's value on
    the voxels of tracks that occupy at least ``min_duration`` planes, ``fill`` elsewhere (on the background too), in the
    caller's class, dimension order and dtype.  ``ridges``, ``reach``, ``connectivity``, ``cyclic`` and what a track is: as
    for ``track_ridges`` -- a short-lived ridge that merges into a lasting one is part of its track and stays."""
    eng, record, out, _, connectivity, reach, min_duration = _ridge_record(ridges, connectivity, reach, min_duration)
    return out(eng.filter_tracks(record, min_duration=min_duration, connectivity=connectivity, cyclic=cyclic, reach=reach, fill=fill),
               keep_dtype=True)


def _local_threshold(da, block_size, method, offset, mode, param, cyclic, want):
    """What the two local-threshold functions share: skimage's argument rules, the field sorted as ``filter_ridges`` sorts it,
    one ``Engine.local_threshold`` call, and the way back to the caller's class and dimension order."""
    if isinstance(block_size, (int, np.integer)):
        blocks = (int(block_size),) * 2
    else:
        blocks = tuple(block_size)
        if len(blocks) != 2 or not all(isinstance(b, (int, np.integer)) for b in blocks):
            raise ValueError(f"block_size {block_size!r}: an odd int or a (latitude, longitude) pair of odd ints")
    if any(b % 2 == 0 for b in blocks):
        raise ValueError(f"block_size {block_size!r}: must be odd (skimage.filters.threshold_local's rule)")
    if any(b < 1 for b in blocks):
        raise ValueError(f"block_size {block_size!r}: >= 1")
    if method != 'gaussian':
        raise NotImplementedError(f"method {method!r}: only 'gaussian' (skimage's default) runs on the device")
    if mode != 'reflect':
        raise NotImplementedError(f"mode {mode!r}: only 'reflect' (skimage's default); cyclic=True makes longitude periodic")
    sigma = tuple((b - 1) / 6.0 for b in blocks) if param is None else param
    dims = tuple(da.dims)
    lead = [d for d in dims if d not in ("latitude", "longitude")]
    if len(lead) > 1 or len(dims) - len(lead) != 2:
        raise ValueError("da: dims (latitude, longitude) and at most one more")
    order = (*lead, "latitude", "longitude")
    lat, lon = _coord(da, "latitude"), _coord(da, "longitude")
    ilat, ilon = np.argsort(lat, kind="stable"), np.argsort(lon, kind="stable")
    v = np.asarray(da.transpose(*order).values)
    v = v if v.dtype in (np.float32, np.float64) else v.astype(np.float64)
    v = np.ascontiguousarray(v[..., ilat, :][..., ilon])
    coords = {"latitude": lat[ilat], "longitude": lon[ilon]}
    if lead:
        coords[lead[0]] = _coord(da, lead[0])
    res = get_engine().local_threshold(v, sigma, offset=offset, cyclic=cyclic, want=(want,))[want]
    res = _to_np(res)
    res = res.astype(bool) if want == "mask" else res
    return _make(da, res, order, coords, getattr(da, "name", None)).transpose(*dims)


def threshold_local(da, block_size=3, method='gaussian', offset=0, mode='reflect', param=None, cval=0, cyclic=False):
    """The adaptive threshold of ``skimage.filters.threshold_local`` on the device (``Engine.local_threshold``): the call
    LCS/area_of_influence.py:194 makes, ``threshold_local(ftle_local.values, block_size=301, offset=-.8)``.  skimage's
    signature plus ``cyclic``.

    scikit-image is not a dependency of this project, so the rule is restated from its documented definition: with
    ``method='gaussian'`` the threshold of a pixel is the Gaussian-weighted mean of its neighbourhood minus ``offset``, i.e.
    ``scipy.ndimage.gaussian_filter(image, sigma, mode='reflect') - offset`` with ``sigma = (block_size - 1) / 6`` (or
    ``param``, when given), truncated at 4 sigma as scipy truncates it.  ``block_size`` is an odd int or a ``(latitude,
    longitude)`` pair of odd ints -- an even one raises ``ValueError`` as in skimage -- and a block of 1 leaves its axis
    unfiltered.  The other methods (``'mean'``, ``'median'``, ``'generic'``) and boundary modes raise
    ``NotImplementedError``; ``cval`` belongs to ``mode='constant'`` and is accepted for the signature.  The radius
    ``int(4 sigma + 0.5)`` may be many times the plane but not above 256 (``block_size`` up to 385).

    ``da`` is a labelled array over ``latitude`` and ``longitude`` (sorted ascending here, as ``filter_ridges`` sorts), 2-D,
    or 3-D with one more dimension (time, member): every plane then gets its own threshold -- never smoothed across time --
    all of them in the same kernel launches.  ``cyclic``: longitude is periodic (a global axis) instead of reflected.

    Returns the float64 threshold in the caller's class and dimension order."""
    return _local_threshold(da, block_size, method, offset, mode, param, cyclic, "threshold")


def above_local_threshold(da, block_size, offset=0, param=None, cyclic=False):
    """``da > threshold_local(da, block_size, offset=offset, param=param, cyclic=cyclic)`` in one call: the driver's
    ``binary_local = ftle_local > local_thresh`` (LCS/area_of_influence.py:195), the comparison fused into the Gaussian's last
    pass so that no threshold plane is written or read back.  A NaN in ``da`` or in its threshold gives ``False``.

    Returns the boolean mask in the caller's class and dimension order."""
    return _local_threshold(da, block_size, 'gaussian', offset, 'reflect', param, cyclic, "mask")


def relative_vorticity(u, v, cyclic=False, deviation='none', radius=6371000.0):
    """Relative vorticity of a wind on the sphere, ``(dv/dlambda - d(u cos phi)/dphi) / (R cos phi)`` in 1/s, on the device
    (``Engine.vorticity``): centred differences, second-order one-sided ones at the first and last row (and column, unless
    ``cyclic``: then centred across the seam), the adjacent row's mean on a pole row, NaN where a stencil holds a non-finite
    wind.  ``u`` and ``v`` are labelled arrays over ``latitude`` and ``longitude`` -- uniformly spaced; sorted ascending here, as
    ``filter_ridges`` sorts -- 2-D, or 3-D with one more dimension (time).  ``deviation``: ``'none'``, ``'domain'`` (subtract
    each level's ``cos phi``-weighted mean: the field ``LCS.lavd`` integrates) or one value per level to subtract.

    Returns the vorticity in the caller's class with dims ``(time, latitude, longitude)`` (``(latitude, longitude)`` for a
    2-D wind), named ``'vorticity'``."""
    dims = tuple(u.dims)
    if set(dims) != set(v.dims):
        raise ValueError("u and v dims are different")
    lead = [d for d in dims if d not in ("latitude", "longitude")]
    if len(lead) > 1 or len(dims) - len(lead) != 2:
        raise ValueError("u, v: dims (latitude, longitude) and at most one more")
    order = (*lead, "latitude", "longitude")
    lat, lon = _coord(u, "latitude"), _coord(u, "longitude")
    if not (np.array_equal(lat, _coord(v, "latitude")) and np.array_equal(lon, _coord(v, "longitude"))):
        raise ValueError("u and v coordinates differ")
    ilat, ilon = np.argsort(lat, kind="stable"), np.argsort(lon, kind="stable")

    def planes(da):
        a = np.asarray(da.transpose(*order).values)
        a = a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)
        a = np.ascontiguousarray(a[..., ilat, :][..., ilon])
        return a if lead else a[None]
    uu, vv = planes(u), planes(v)
    lat, lon = lat[ilat], lon[ilon]
    Engine.checked_vorticity_options(uu.shape, vv.shape, lat, lon, deviation, radius)
    res = _to_np(get_engine().vorticity(uu, vv, lat, lon, cyclic=cyclic, deviation=deviation, radius=radius)["omega"])
    coords = {"latitude": lat, "longitude": lon}
    if lead:
        coords[lead[0]] = _coord(u, lead[0])
    return _make(u, res if lead else res[0], order, coords, "vorticity")


def trajectory_density(x, y, lat, lon, weights=None, values=None, cyclic=False):
    """Trajectories the caller already has, binned into a residence map on the device (``Engine.footprint_update``): how long
    the parcels stayed over each cell of the grid ``lat`` x ``lon`` (cell centres in degrees, uniform and ascending; ``cyclic``:
    the columns wrap) and what they carried there.  ``x`` and ``y`` are the ``(time, latitude, longitude)`` longitudes and
    latitudes of ``parcel_propagation(..., return_traj=True)`` -- labelled arrays, or plain arrays with the levels first.
    ``weights``: non-negative numbers on the seed grid, NaN and 0 leaving a parcel out; None: every parcel counts once.
    ``values``: what the parcels carry, of ``x``'s shape (``parcel_propagation``'s ``c``).

    Returns ``(residence_count, mean_value)`` on ``(latitude, longitude)`` of the target grid, float64, in ``x``'s class:
    ``residence_count`` is the trapezoid rule over the levels in units of one step -- the first and the last level count
    half -- so multiply it by the step for a time; with ``weights`` each visit counts by the parcel's weight (to within 2^-21
    of the largest).  ``mean_value`` is the mean of ``values`` over the visits to each cell (to within ``max |values|`` 2^-31),
    NaN where there were none; None without ``values``.  Positions outside the grid, and NaN, are left out."""
    def levels_first(a, what):
        if hasattr(a, "dims"):
            lead = [d for d in a.dims if d not in ("latitude", "longitude")]
            if len(lead) != 1 or len(a.dims) != 3:
                raise ValueError(f"{what}: dims (time, latitude, longitude)")
            a = a.transpose(lead[0], "latitude", "longitude")
        v = np.asarray(getattr(a, "values", a))
        return np.ascontiguousarray(v if v.dtype in (np.float32, np.float64) else v.astype(np.float64))
    tx, ty = levels_first(x, "x"), levels_first(y, "y")
    if tx.ndim < 2 or tx.shape != ty.shape or tx.shape[0] < 2:
        raise ValueError("x and y: one shape, (levels, ...), at least two levels")
    lat, lon = np.asarray(getattr(lat, "values", lat), dtype=np.float64), np.asarray(getattr(lon, "values", lon), dtype=np.float64)
    Engine.checked_footprint_grid(lat, lon, cyclic)
    q, wscale = Engine.footprint_weights(getattr(weights, "values", weights), tx.shape[1:])
    c = c_scale = None
    if values is not None:
        c = levels_first(values, "values")
        if c.shape != tx.shape:
            raise ValueError("values: the shape of x")
        top = np.abs(c[np.isfinite(c)]).max() if np.isfinite(c).any() else 0.0
        c_scale = float(1 << 30) / float(top) if top > 0 else 1.0
    dtype = common_dtype(tx, ty, c)
    eng = get_engine()
    acc = eng.footprint_update(tx.astype(dtype), ty.astype(dtype), lat, lon, 0, True, q, None if c is None else c.astype(dtype), c_scale,
                               None, cyclic)
    count = _to_np(acc["hits"]).astype(np.float64) * 0.5 if weights is None else (_to_np(acc["mass"]).astype(np.float64) * wscale) * 0.5
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = None if c is None else (_to_np(acc["csum"]).astype(np.float64) / _to_np(acc["chits"]).astype(np.float64)) / c_scale
    if not hasattr(x, "dims"):
        return count, mean
    coords = {"latitude": lat, "longitude": lon}
    return (_make(x, count, ("latitude", "longitude"), coords, "residence_count"),
            None if mean is None else _make(x, mean, ("latitude", "longitude"), coords, getattr(values, "name", None) or "mean_value"))


def Inverse_weighted_interpolation(x, y, z, xi, yi, power=2):
    """Values ``z`` known at longitudes ``x`` and latitudes ``y`` (degrees), interpolated to the points ``(xi, yi)`` by
    inverse-distance weighting with great-circle distances: ``u = sum(z / d**power) / sum(1 / d**power)``.  Signature of
    LCS/tools.py:285 (an all-pairs numba loop there); returns an array of ``len(xi)`` in ``z``'s dtype (float32 / float64 kept,
    anything else float64), where the reference returns a list.

    Two departures from the reference, whose function is broken as written: its haversine distance calls ``np.arctan(sqrt(a),
    sqrt(1 - a))`` where it means ``arctan2`` (the second argument is numpy's ``out=``) -- the distance here is the true
    great-circle distance, ``2 R asin(chord / 2)`` as everywhere in this package (``Engine.idw_interp`` states every rounding)
    --, and a point ``(xi, yi)`` that coincides with a source gives ``inf / inf = NaN`` there and that source's value here (the
    mean of several), the limit of the weighting.  The result does not depend on the radius: the reference's 6378.1 km and this
    package's 6371 km give one field.  A NaN in ``z`` leaves its source out."""
    x, y, xi, yi = (np.asarray(getattr(a, "values", a)) for a in (x, y, xi, yi))
    z = np.asarray(getattr(z, "values", z))
    plan = Engine.idw_plan(x, y, z.shape, xi, yi, False, power)               # every refusal, before a device
    if z.ndim != 1 or len(plan["shape"]) != 1:
        raise ValueError("x, y, z and xi, yi: one-dimensional")
    return _to_np(get_engine().idw_interp(x, y, z, xi, yi, power=power))


def xr_idx_interp(ds_y_for_spline, lon, lat, p=2, max_distance=None, radius=6371000.0, return_weight=False, return_count=False):
    """Grid the values of a labelled array of scattered points -- one ``points``-like dimension along which it carries
    ``longitude`` and ``latitude`` coordinates in degrees -- onto ``lat`` x ``lon`` by inverse-distance weighting on the
    sphere.  Signature of LCS/tools.py:302 with four keywords more; the result has dims ``(latitude, longitude)`` on the
    coordinates given (in the order given, sorted or not), in the class and the dtype of the input.  A leading dimension in
    front of the points (time, tracer) is a stack of fields on the same positions: every plane is gridded on its own, the
    geometry of a pair evaluated once for all of them, and the result is ``(that dimension, latitude, longitude)``.

    ``p``: the power of the distance, ``0 < p <= 16``.  ``max_distance`` (in the unit of ``radius``, metres on the default
    Earth): only sources within that great-circle distance contribute, a node without one is NaN, and the search is cut to
    the sources within the bound's band of latitudes; None: every source contributes to every node, as in the reference.
    ``return_weight``: also ``sum(1 / d**p)``, float64 (``+inf`` where a source lies on the node).  ``return_count``: also the
    int32 number of sources within reach of each node, dims ``(latitude, longitude)``.  Returns the field, then the weight,
    then the count, as asked for.

    The departures from the reference are those of ``Inverse_weighted_interpolation``: the true great-circle distance where
    the reference's haversine misuses ``arctan``, and the source's own value, not NaN, where a source lies on a node.  NaN
    values are left out, plane by plane; sources whose coordinates are not finite, or beyond the poles, altogether."""
    da = ds_y_for_spline
    dims = tuple(da.dims)
    if len(dims) not in (1, 2):
        raise ValueError(f"dims {dims}: one dimension of points, and at most one in front of it")
    x, y = _coord(da, "longitude"), _coord(da, "latitude")
    # the dimension the coordinates run along: xarray names it; a class that does not is asked for the (last) dimension of
    # their length
    along = tuple(getattr(da["longitude"], "dims", ()))
    fits = [d for d, n in zip(dims, np.shape(da.values)) if n == x.size]
    points = along[0] if len(along) == 1 and along[0] in dims else fits[-1] if fits else dims[-1]
    lead = [d for d in dims if d != points]
    v = np.asarray(da.transpose(*lead, points).values)
    v = v if v.dtype in (np.float32, np.float64) else v.astype(np.float64)
    lon, lat = np.asarray(getattr(lon, "values", lon)), np.asarray(getattr(lat, "values", lat))
    Engine.idw_plan(x, y, v.shape, lon, lat, True, p, radius, max_distance)    # every refusal, before a device
    got = get_engine().idw_interp(x, y, v, lon, lat, grid=True, power=p, radius=radius, max_distance=max_distance,
                                  return_weight=return_weight, return_count=return_count)
    got = got if isinstance(got, tuple) else (got,)
    order, coords = (*lead, "latitude", "longitude"), {"latitude": lat, "longitude": lon}
    if lead and lead[0] in da.coords:
        coords[lead[0]] = _coord(da, lead[0])
    name = getattr(da, "name", None)
    out = [_make(da, _to_np(t), order, coords, name) for t in got[:1 + bool(return_weight)]]
    if return_count:
        out.append(_make(da, _to_np(got[-1]), ("latitude", "longitude"), {"latitude": lat, "longitude": lon}, name))
    return out[0] if len(out) == 1 else tuple(out)
