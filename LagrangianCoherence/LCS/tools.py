"""``from LagrangianCoherence.LCS.tools import ...`` -- the hot-path helpers, HIP-backed."""
from lagrangiancoherence_amd.tools import (above_local_threshold, derivative_spherical_coords, dilate_ridges,  # noqa: F401
                                           distance_to_ridges, filter_ridges, find_ridges_spherical_hessian,
                                           fourth_order_derivative, persistent_ridges, ridge_lines, ridge_properties, skeletonize_ridges,
                                           threshold_local, track_ridges, xr_map_coordinates)
