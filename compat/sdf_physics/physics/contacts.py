"""`sdf_physics.physics.contacts`: the SDF contact handler (contacts.py:31-141) on the device."""
from diffsdfsim_amd.physics2d.sdf_contacts import SDFContactHandler  # noqa: F401
