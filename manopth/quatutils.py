"""`manopth.quatutils` drop-in (reference: pose_data_optimize/manopth/manopth/quatutils.py): the two functions the optimiser's
hand model needs."""
from renderih_amd.quat_mano import normalize_quaternion, quaternion_to_rotation_matrix  # noqa: F401
