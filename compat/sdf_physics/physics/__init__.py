"""`sdf_physics.physics` of the reference (its 2-D SDF layer), served by the MI355X build (see compat/README.md)."""
