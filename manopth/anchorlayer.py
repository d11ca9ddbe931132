"""`manopth.anchorlayer` drop-in (reference: pose_data_optimize/manopth/manopth/anchorlayer.py) on csrc/rih_anchor.hip."""
from renderih_amd.quat_mano import FusedAnchorLayer as AnchorLayer  # noqa: F401
from renderih_amd.quat_mano import AnchorLayer as TorchAnchorLayer  # noqa: F401
