"""Drop-in import path for the pose optimiser's `manopth` package (reference: pose_data_optimize/manopth/manopth):
`manopth.manolayer.ManoLayer` in quaternion mode, `manopth.anchorlayer.AnchorLayer` and two functions of `manopth.quatutils`
resolve to the MI355X-native implementation in renderih_amd/quat_mano.py; `manopth.axislayer`, `manopth.rodrigues_layer` and
the rest resolve to the reference checkout behind this repository."""

import os as _os
import sys as _sys

name = 'manopth'

# Keep the reference's own sub-modules of this package importable when its checkout is ALSO on sys.path (behind this
# repository): a regular package shadows same-named directories further down the path, so they are appended to
# __path__ here -- modules defined in this directory win, everything else resolves to the reference.
for _p in list(_sys.path):
    _cand = _os.path.join(_p or '.', *__name__.split('.'))
    if _os.path.isdir(_cand) and _os.path.abspath(_cand) != _os.path.dirname(_os.path.abspath(__file__)) \
            and _cand not in __path__:
        __path__.append(_cand)
