"""The fp16 backbone's convolution kernels (csrc/rih_half.hip) away from unit scale and on the wide halo tiles: ONE list of
cases, run on the GPU by tests/test_gpu_half_range.py and on the host build of the kernels by tests/test_half.py.  Every case is
test_half.conv_case with bar='range' (fp64 reference of the same fp16 operands, tests/test_half.py::check_range), both output
types against one reference, and the plan code rih_hconv_plan must give for it -- so a case tests the kernel it names."""
import os

from renderih_amd.half import PLAN_BASE as B_, PLAN_BN128 as BN128, PLAN_HALO as HALO, PLAN_REGS as REGS, PLAN_TW16 as TW16

# regime -> keywords of conv_case.  `res`: the regime wants a residual (given to the kernels that take one: the halo kernels do
# not, rih_hconv would hand the call to the implicit GEMM); `relu`: overrides the kernel's own setting
REGIMES = {
    'sub_w_partial': dict(gamma=(1e-3, 2e-3), guard='sub_w_partial'),      # folded weights partly fp16 subnormals
    'sub_w_all': dict(gamma=(1e-5, 2e-5), guard='sub_w_all'),              # ... all of them
    'tiny_var': dict(var=(1e-8, 1e-6)),                                    # dead channels: scale = gamma / sqrt(eps) ~ 300
    'small_x': dict(xs=1e-3, rs=1e-3, res=True),
    'sub_x': dict(xs=1e-4, guard='sub_x'),                                 # activations mostly fp16 subnormals
    'big_x': dict(xs=300.0),
    'saturate': dict(xs=3000.0, ws=8.0, res=True, relu=False, guard='saturate'),   # clamp_h of the epilogue
    'zero_gamma': dict(zero_gamma=(0, 7, 13, 19)),                         # the output of these channels is exactly the shift
}

# kernel -> (N, H, W, Cin, Cout, k, stride, pad, order, relu, res), extra keywords, takes a residual,
#           plan by switch: default, RIH_HCONV_GLDS=0, RIH_HCONV_HALO=0, RIH_HCONV_BN=128
KERNELS = {
    'gemm64': ((1, 8, 8, 64, 64, 1, 1, 0, 'conv-bn', True, False), {}, True, (B_, B_ | REGS, B_, B_)),
    'gemm128': ((1, 8, 8, 64, 128, 3, 2, 1, 'conv-bn', True, False), {}, True,
                (B_ | BN128, B_ | BN128 | REGS, B_ | BN128, B_ | BN128)),
    # one k-tile and a wide output: 128 x 64 tiles by the occupancy rule, 128 x 128 when RIH_HCONV_BN=128 switches it off
    'gemm_one_ktile': ((1, 8, 8, 64, 256, 1, 1, 0, 'conv-bn', True, True), {}, True, (B_, B_ | REGS, B_, B_ | BN128)),
    'ragged': ((1, 8, 8, 64, 20, 1, 1, 0, 'conv-bn', True, True), {}, True, (B_, B_ | REGS, B_, B_)),
    # Conv -> ReLU -> BN: gamma / var act on post_scale / post_shift, the weights stay at unit scale
    'relu_bn': ((1, 6, 6, 96, 64, 3, 1, 1, 'conv-relu-bn', True, False), {}, True, (B_, B_ | REGS, B_, B_)),
    'stem': ((1, 20, 20, 8, 64, 7, 2, 3, 'conv-bn', True, False), dict(cin_w=3), True, (B_, B_ | REGS, B_, B_)),
    'halo32x64': ((1, 8, 32, 64, 64, 3, 1, 1, 'conv-bn', True, False), {}, False, (B_ | HALO, B_ | HALO, B_, B_ | HALO)),
    'halo16x64': ((1, 16, 16, 128, 128, 3, 1, 1, 'conv-bn', True, False), {}, False,
                  (B_ | HALO | TW16, B_ | HALO | TW16, B_ | BN128, B_ | HALO | TW16)),
}

# the 128-channel halo tiles are chosen from 256 workgroups on: patches * Cout / 128 >= 256
WIDE = {
    'halo32x128': ((1, 64, 256, 64, 512, 3, 1, 1, 'conv-bn', True, False), {}, False,
                   (B_ | HALO | BN128, B_ | HALO | BN128, B_ | BN128, B_ | HALO | BN128)),
    'halo16x128': ((1, 64, 272, 64, 512, 3, 1, 1, 'conv-bn', True, False), {}, False,
                   (B_ | HALO | TW16 | BN128, B_ | HALO | TW16 | BN128, B_ | BN128, B_ | HALO | TW16 | BN128)),
    'halo32x64_below_rule': ((1, 56, 256, 64, 512, 3, 1, 1, 'conv-bn', True, False), {}, False,
                             (B_ | HALO, B_ | HALO, B_ | BN128, B_ | HALO)),
    'halo32x128_two_chunks': ((1, 64, 256, 128, 512, 3, 1, 1, 'conv-bn', True, False), {}, False,
                              (B_ | HALO | BN128, B_ | HALO | BN128, B_ | BN128, B_ | HALO | BN128)),
}
WIDE_REGIMES = ('unit', 'sub_w_partial', 'saturate')

CASES = [(k, r) for k in KERNELS for r in REGIMES]
WIDE_CASES = [(k, r) for k in WIDE for r in WIDE_REGIMES]


def switch():
    """Which of the library's per-process switches this interpreter runs under (index into a kernel's plans)."""
    off = lambda k: os.environ.get(k, '').startswith('0')
    return 1 if off('RIH_HCONV_GLDS') else 2 if off('RIH_HCONV_HALO') else 3 if os.environ.get('RIH_HCONV_BN') == '128' else 0


def run_case(conv_case, dev, kernel, regime, run=True):
    """One (kernel, regime) through conv_case: both output types, plan asserted.  Returns conv_case's measurements."""
    args, extra, takes_res, plans = (KERNELS.get(kernel) or WIDE[kernel])
    kw = dict(REGIMES.get(regime, {}), **extra)
    args = list(args)
    if kw.pop('res', False) and takes_res:
        args[10] = True
    if 'relu' in kw:
        args[9] = kw.pop('relu')
    if args[8] != 'conv-bn' and kw.get('guard') in ('sub_w_partial', 'sub_w_all'):
        del kw['guard']                               # the scale is not folded into these weights
    seed = 100 + 16 * sorted(list(KERNELS) + list(WIDE)).index(kernel) + (['unit'] + list(REGIMES)).index(regime)
    return conv_case(dev, *args, 'both', seed=seed, bar='range', expect_plan=plans[switch()], run=run,
                     what='%s/%s' % (kernel, regime), **kw)


def run_all(conv_case, dev):
    """The list once under one of the per-process switches (the child interpreters): every small case, and the wide shapes
    where the switch changes their kernel -- elsewhere the child would repeat the parent's launch on the parent's data -- one
    shape per (kernel, Cin, Cout): without the halo kernels the wide shapes differ only in their pixel count."""
    sw, seen, wide = switch(), set(), []
    for k, (args, _, _, plans) in WIDE.items():
        if plans[sw] != plans[0] and (plans[sw], args[3], args[4]) not in seen:
            seen.add((plans[sw], args[3], args[4]))
            wide += [(k, r) for r in WIDE_REGIMES]
    return {(k, r): run_case(conv_case, dev, k, r) for k, r in CASES + wide}
