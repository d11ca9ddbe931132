"""`utils.vis_utils` drop-in (reference: utils/vis_utils.py): the HIP two-hand renderer."""
from renderih_amd.render import *  # noqa: F401,F403
from renderih_amd.render import Renderer, mano_renderer, mano_two_hands_renderer  # noqa: F401
