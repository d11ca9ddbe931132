"""Build librenderih_amd.so (hand-written HIP kernels + C ABI) for gfx950, in-tree.

`hipcc --offload-arch=gfx950` cross-compiles without a GPU.  The .so is git-ignored but travels to the
GPU box with the repo snapshot.  Each source is compiled to its own object (in parallel, only when it or a header is
newer than the object), then linked; nothing is rebuilt when the library is newer than every source.
"""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
OBJ = os.path.join(CSRC, '_obj')
LIB = os.path.join(HERE, 'librenderih_amd.so')
# Kernel variants that were measured and refuted in rounds 2-5 (P3 GEMM, row chain, tile 4, pre-split operands, the BatchNorm-backward
# epilogue) live on the git branch `experiments-r05`, not in this tree.
SOURCES = ['rih_gemm.hip', 'rih_conv3.hip', 'rih_elem.hip', 'rih_mano.hip', 'rih_loss.hip', 'rih_metrics.hip',
           'rih_pose.hip', 'rih_attn.hip', 'rih_flash.hip', 'rih_half.hip', 'rih_input.hip', 'rih_sdf.hip',
           'rih_render.hip', 'rih_mano_loss.hip', 'rih_sdf_loss.hip', 'rih_anchor.hip', 'rih_pose_prior.hip', 'rih_pose_opt.hip',
           'rih_contact.hip', 'rih_nature.hip', 'rih_collision.hip', 'rih_joint_fit.hip', 'rih_pose_convert.hip',
           'rih_aux.hip', 'rih_demo.hip']
HEADERS = ['rih_procrustes.h', 'rih_pose_math.h', 'rih_hash.h', 'rih_e2.h', 'rih_reduce.h', 'rih_mesh_terms.h']
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-result',
         # hipcc's SLP pass packs neighbouring f32 adds into v_pk_add_f32, which issues at a fraction of the scalar
         # rate next to MFMAs (MI355X_MICROARCH.md, cycle constants): keep the split arithmetic scalar
         '-fno-slp-vectorize']


def hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return 'hipcc'


def _deps():
    return [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.join(HERE, '..', 'include', 'renderih_amd.h')]


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in _deps()) or _flags_changed()


def _flags_stamp():
    import hashlib
    return hashlib.sha256(' '.join(FLAGS + SOURCES).encode()).hexdigest()[:16]


def _flags_changed():
    try:
        with open(os.path.join(OBJ, 'flags.stamp')) as fh:
            return fh.read().strip() != _flags_stamp()
    except OSError:
        return True


def build(force=False, verbose=True):
    if not force and not needs_build():
        return LIB
    os.makedirs(OBJ, exist_ok=True)
    force = force or _flags_changed()       # objects compiled with other FLAGS are stale whatever their mtime
    hdr_t = max(os.path.getmtime(d) for d in _deps()[len(SOURCES):])
    jobs = []
    for s in SOURCES:
        src, obj = os.path.join(CSRC, s), os.path.join(OBJ, s + '.o')
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), hdr_t):
            jobs.append([hipcc()] + FLAGS + ['-c', src, '-o', obj])

    def run(cmd):
        if verbose:
            print('[renderih_amd] building:', ' '.join(cmd), flush=True)
        subprocess.check_call(cmd)
    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    run([hipcc(), '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + [os.path.join(OBJ, s + '.o') for s in SOURCES])
    with open(os.path.join(OBJ, 'flags.stamp'), 'w') as fh:
        fh.write(_flags_stamp())
    return LIB


if __name__ == '__main__':
    build(force=True)
