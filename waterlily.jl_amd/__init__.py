"""waterlily.jl_amd — MI355X (gfx950) backend for WaterLily's time-step hot path.

Host-side mirror (Python) of the reference's Flow / AbstractPoisson / Simulation surface for that path, over
hand-written HIP kernels behind a flat C ABI (include/wlhip.h, libwlhip.so).  No CPU fallback exists.
"""
from ._lib import LIB_PATH, SIGNATURES, WlError, lib  # noqa: F401
from .core import (BC_, BC_terms_, CDS, QUICK, VANLEER, L2, accel_terms_, exitBC_, inside, jl_zeros, loc, perBC_, tabulate, to_device, to_host)  # noqa: F401
from .flow import BDIM_, CFL, Flow, conv_diff_, mom_correct_, mom_predict_, mom_project_, mom_step_, scale_u_, sgs, sgs_, udf_  # noqa: F401
from .poisson import (pcg_, poisson_solver_, GaussSeidelRB_, Jacobi_, L1, Linf, MultiLevelPoisson, Poisson, increment_, mult_, norms, prolongate_,  # noqa: F401
                      residual_, restrict_, restrictL_, set_diag_, smooth_, update_)
from .metrics import (MeanFlow, curl_, flow_fields_, flow_stats, helicity_, ke_, lambda2_, load_checkpoint, omega_, omega_mag_, omega_theta_,  # noqa: F401
                      save_checkpoint)
from .interp import advect_, interp, interp_  # noqa: F401
from .simulation import (FusedSimulation, Simulation, measure_, pressure_force, pressure_moment, viscous_force,  # noqa: F401
                         viscous_moment)
from . import bodies  # noqa: F401,E402
from .bodies import Body, RigidMap, SdfLattice, SetBody, mesh_band, mesh_body, read_stl, setmap, weld  # noqa: F401,E402
