"""`manopth.manolayer` drop-in (reference: pose_data_optimize/manopth/manopth/manolayer.py): the quaternion mode on the fused
HIP kernels.  `ManoLayer` takes manopth's constructor (hocontact/postprocess/geo_optimizer_both_batch.py:54-79) and reads
MANO_RIGHT.pkl / MANO_LEFT.pkl under `mano_root`; every other rotation mode raises NotImplementedError."""
import os

from renderih_amd.quat_mano import FusedQuatManoLayer, QuatManoLayer  # noqa: F401
from renderih_amd.quat_mano import normalize_quaternion, quaternion_to_rotation_matrix  # noqa: F401


class ManoLayer(FusedQuatManoLayer):
    def __init__(self, center_idx=None, flat_hand_mean=True, ncomps=6, side='right', mano_root='mano/models', use_pca=True,
                 root_rot_mode='axisang', joint_rot_mode='axisang', robust_rot=False, return_transf=False,
                 return_full_pose=False):
        if side not in ('right', 'left'):
            raise ValueError("side must be 'right' or 'left'; got %r" % (side,))
        self.mano_path = os.path.join(mano_root, 'MANO_RIGHT.pkl' if side == 'right' else 'MANO_LEFT.pkl')
        super().__init__(self.mano_path, side=side, center_idx=center_idx, return_transf=return_transf,
                         return_full_pose=return_full_pose, joint_rot_mode=joint_rot_mode, root_rot_mode=root_rot_mode,
                         use_pca=use_pca, flat_hand_mean=flat_hand_mean)
        self.robust_rot = robust_rot
