"""``from LagrangianCoherence.LCS.tools import ...`` -- the hot-path helpers, HIP-backed."""
from lagrangiancoherence_amd.tools import (derivative_spherical_coords, dilate_ridges, distance_to_ridges, filter_ridges,  # noqa: F401
                                           find_ridges_spherical_hessian, fourth_order_derivative, skeletonize_ridges,
                                           xr_map_coordinates)
