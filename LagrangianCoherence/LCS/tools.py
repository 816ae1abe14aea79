"""``from LagrangianCoherence.LCS.tools import ...`` -- the hot-path helpers, HIP-backed."""
from lagrangiancoherence_amd.tools import (Inverse_weighted_interpolation, above_local_threshold,  # noqa: F401
                                           derivative_spherical_coords, dilate_ridges,
                                           distance_to_ridges, filter_ridges, find_ridges_spherical_hessian,
                                           fourth_order_derivative, persistent_ridges, relative_vorticity, ridge_lines, ridge_properties, ridge_transects,
                                           skeletonize_ridges,
                                           threshold_local, track_ridges, trajectory_density, xr_idx_interp, xr_map_coordinates)
