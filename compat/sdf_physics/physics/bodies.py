"""`sdf_physics.physics.bodies` of the reference: the 2-D SDF bodies (bodies.py:28-493) of diffsdfsim_amd.physics2d."""
from diffsdfsim_amd.physics2d.sdf_bodies import SDF, SDFBowl, SDFCircle, SDFGrid, SDFRect  # noqa: F401
