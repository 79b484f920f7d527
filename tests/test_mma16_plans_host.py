"""CPU: the plans behind the bf16 gradient / forward entry points (csrc/mma16_common.h: the parameter-layout check,
the slab split; csrc/conv_wgrad_common.h, conv_wgrad_bf16.hip's two forms, conv_wgrad_kxk.hip, conv_dgrad_bf16.hip,
conv_kxk_bf16.hip, deconv_grad_bf16.hip, bnrelu_conv_bf16.hip) return what they returned before the shared helpers
existed.  tests/golden/mma16_plans.json holds, for the table of descriptors
below, the value of every *_check / *_slabs / *_workspace_elems / *_pack_elems entry point as the library answered
before the helpers moved (`python tests/test_mma16_plans_host.py --record` rewrites it from the library in the
tree: only for a change that is meant to alter a plan)."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mma16_plans.json')

# family -> (descriptor class, defaults, [(entry point, extra arguments)])
FAMILIES = {
    'wgrad': ('ConvWgradDesc', dict(B=2, Cin=24, Cout=16, H=20, W=20, K=3, pad=1),
              [('iiseg_conv_wgrad_bf16_slabs', ()), ('iiseg_conv_wgrad_bf16_workspace_elems', ()),
               ('iiseg_conv_wgrad_bf16_co16_slabs', ()), ('iiseg_conv_wgrad_bf16_co16_workspace_elems', ()),
               ('iiseg_conv_wgrad_check', ()), ('iiseg_conv_wgrad_slabs', (4,)), ('iiseg_conv_wgrad_slabs', (8,)),
               ('iiseg_conv_wgrad_workspace_elems', (4,)), ('iiseg_conv_wgrad_workspace_elems', (8,))]),
    'dgrad': ('ConvDgradDesc', dict(B=2, Cin=24, Cout=16, H=20, W=20, K=3, pad=1),
              [('iiseg_conv_dgrad_bf16_check', ()), ('iiseg_conv_dgrad_bf16_pack_elems', ())]),
    'kxk_wgrad': ('ConvWgradKxKDesc', dict(B=2, Cin=24, Cout=16, H=13, W=13, K=7),
                  [('iiseg_conv_wgrad_kxk_bf16_check', ()), ('iiseg_conv_wgrad_kxk_bf16_slabs', ()),
                   ('iiseg_conv_wgrad_kxk_bf16_workspace_elems', ()), ('iiseg_conv_wgrad_kxk_check', ()),
                   ('iiseg_conv_wgrad_kxk_slabs', (4,)), ('iiseg_conv_wgrad_kxk_slabs', (8,)),
                   ('iiseg_conv_wgrad_kxk_workspace_elems', (4,)), ('iiseg_conv_wgrad_kxk_workspace_elems', (8,))]),
    'kxk_dgrad': ('ConvDgradDesc', dict(B=2, Cin=24, Cout=16, H=7, W=7, K=7),
                  [('iiseg_conv_dgrad_kxk_bf16_check', ()), ('iiseg_conv_dgrad_kxk_bf16_slabs', ()),
                   ('iiseg_conv_dgrad_kxk_bf16_workspace_elems', ()), ('iiseg_conv_dgrad_kxk_bf16_pack_elems', ())]),
    'kxk_fwd': ('ConvFwdKxKDesc', dict(B=2, Cin=24, Cout=16, H=13, W=13, K=7, relu=1),
                [('iiseg_conv_fwd_kxk_bf16_check', ()), ('iiseg_conv_fwd_kxk_bf16_slabs', ()),
                 ('iiseg_conv_fwd_kxk_bf16_workspace_elems', ())]),
    'deconv': ('DeconvDesc', dict(B=2, Cin=24, Cout=16, H=10, W=10, K=3, stride=2, OH=21, OW=21),
               [('iiseg_deconv_grad_bf16_check', ()), ('iiseg_deconv_wgrad_bf16_slabs', ()),
                ('iiseg_deconv_wgrad_bf16_workspace_elems', ()), ('iiseg_deconv_dgrad_bf16_workspace_elems', ())]),
    'bnrelu_fwd': ('BnReluConvDesc', dict(B=2, n=24, cap=40, Cout=16, H=20, W=20, out_cap=40, out_c0=24),
                   [('iiseg_bnrelu_conv_fwd_bf16_check', ()), ('iiseg_bnrelu_conv_fwd_bf16_slabs', ()),
                    ('iiseg_bnrelu_conv_fwd_bf16_workspace_elems', ())]),
}

EDGES = (1, 63, 64, 65, 100)                       # around the 64-channel block, and a non-multiple of 16
EDGES16 = (1, 15, 16, 17, 63, 64, 65)              # ... and around the 16-channel block of the later kernels
# what every family gets: the layouts, a channel slice, the channel edges, the refusal branches (one fault each, then
# two at once: the first check that fires answers)
COMMON = [dict(), dict(layout='iohw'), dict(ci0=5, Cin_tot=40), dict(ci0=5, Cin_tot=40, layout='iohw')] + \
         [dict(Cin=c) for c in EDGES] + [dict(Cout=c) for c in EDGES] + \
         [dict(so=7, sc=49), dict(ci0=1, Cin_tot=24), dict(ci0=-1), dict(K=0), dict(K=8), dict(H=0), dict(Cin_tot=65536),
          dict(K=8, so=7, sc=49), dict(H=0, ci0=1, Cin_tot=24), dict(so=7, sc=49, Cout=65536)]
KS = [dict(K=k, H=9, W=11) for k in range(1, 8)] + [dict(K=k, H=k - 1, W=k + 3) for k in range(2, 8)]
TABLE = {
    # min-per-slab clamp (the default map), the target decides, the unsplit grid exceeds the target, a wide padding
    'wgrad': COMMON + [dict(B=4, H=200, W=200), dict(Cin=1024, Cout=1024), dict(Cin=1024, Cout=1024, B=4, H=200, W=200),
                       dict(pad=100, H=4, W=4), dict(pad=0, H=2, W=9)] +
             [dict(Cin=c) for c in (15, 16, 17)] + [dict(Cout=c) for c in (15, 16, 17)] +      # the co16 form's blocks
             [dict(Cin=1024, Cout=16), dict(Cin=300, Cout=16, H=14, W=13), dict(Cin=67, Cout=16, B=3, H=37, W=150)],
    'dgrad': COMMON + [dict(pad=0), dict(accumulate=1), dict(accumulate=2), dict(Cin=512, Cout=512, H=422, W=422)],
    'kxk_wgrad': COMMON + KS + [dict(K=3, Cin=512, Cout=512, B=4, H=66, W=66), dict(K=3, Cin=1024, Cout=1024),
                                dict(K=1, H=37, W=150, B=3), dict(B=10, Cin=512, Cout=4096),
                                dict(B=10, Cin=4096, Cout=4096, K=1, H=1, W=1), dict(x_row=12), dict(x_y0=-1)],
    'kxk_dgrad': COMMON + KS + [dict(B=16, Cin=512, Cout=4096), dict(B=64, H=58, W=58, Cout=512),
                                dict(Cin=33, Cout=130), dict(accumulate=2), dict(K=1, H=37, W=150, B=3)],
    'kxk_fwd': [r for r in COMMON if not set(r) & {'layout', 'ci0', 'Cin_tot', 'so', 'sc'}] + KS +
               [dict(Cin=4096, Cout=4096), dict(B=16, H=70, W=70, Cout=256), dict(relu=2),
                dict(K=1, H=37, W=150, B=3, Cin=512, Cout=21)],
    # the whole (2H + 1) x (2W + 1) map (split: the min-per-slab clamp), the channel edges, a cropped window, one tile,
    # the target decides, the unsplit grid reaches the target; then the refusals in db_plan's order
    'deconv': [dict()] + [dict(Cin=c) for c in EDGES16] + [dict(Cout=c) for c in EDGES16] +
              [dict(oy0=1, ox0=1, OH=20, OW=20), dict(oy0=0, ox0=1, OH=19, OW=17), dict(B=1, H=4, W=16, OH=9, OW=33),
               dict(B=3, H=56, W=56, OH=112, OW=112, oy0=1, ox0=1, Cin=48, Cout=48), dict(Cin=1024, Cout=1024),
               dict(B=0), dict(oy0=-1), dict(B=65536), dict(K=1025), dict(OH=22), dict(ox0=1),
               dict(H=16384, W=16384, OH=32769, OW=32769), dict(K=2, OH=20, OW=20), dict(stride=1, OH=12, OW=12),
               dict(K=4, stride=3, OH=31, OW=31), dict(Cin=65535, Cout=65535),
               dict(B=65535, H=16384, W=16384, OH=9, OW=9), dict(B=0, K=2), dict(K=2, OH=22)],
    # one slab (the min-per-slab clamp), the channel edges (n: the k-tile of 32 as well), the reduction splits, the
    # map alone fills the target, the output behind the channels read and elsewhere; then bc_plan's refusals
    'bnrelu_fwd': [dict()] + [dict(n=c, cap=c + 16, out_cap=c + 16, out_c0=c) for c in EDGES16 + (31, 32, 33)] +
                  [dict(Cout=c, out_cap=24 + c) for c in EDGES16] +
                  [dict(n=256, cap=272, out_cap=272, out_c0=256), dict(n=256, cap=272, out_cap=272, out_c0=256, B=7),
                   dict(n=1000, cap=1000, out_cap=16, out_c0=0, H=7, W=7), dict(H=224, W=224), dict(H=37, W=150, B=3),
                   dict(out_cap=16, out_c0=0),
                   dict(B=0), dict(n=0), dict(Cout=0), dict(W=0), dict(cap=23), dict(out_c0=-1), dict(out_c0=25),
                   dict(B=65536), dict(cap=65536), dict(out_cap=65536), dict(H=16385, W=16384),
                   dict(n=60000, cap=60000, Cout=60000, out_cap=60000, out_c0=0), dict(B=65535, H=16384, W=16384),
                   dict(n=0, out_c0=25), dict(cap=65536, H=16385, W=16384)],
}


def _desc(family, row):
    """The descriptor of a table row: the family's defaults, the row's fields, then what follows from them unless
    the row sets it (Cin_tot, the contiguous x window, 'valid' padding, the strides of the layout)."""
    from iterative_inference_segm_amd import _lib
    cls, defaults, _ = FAMILIES[family]
    d = getattr(_lib, cls)()
    row = dict(row)
    layout = row.pop('layout', 'oihw')
    for k, v in list(defaults.items()) + list(row.items()):
        setattr(d, k, v)
    names = [f[0] for f in d._fields_]
    if 'Cin_tot' in names and 'Cin_tot' not in row:
        d.Cin_tot = d.ci0 + d.Cin
    if 'x_row' in names:
        d.x_row = row.get('x_row', d.W)
        d.x_plane, d.x_image = d.H * d.W, d.Cin * d.H * d.W
    if family == 'kxk_dgrad' and 'pad' not in row:
        d.pad = d.K - 1
    if 'so' in names and 'so' not in row:
        KK = d.K * d.K
        d.so, d.sc = (d.Cin_tot * KK, KK) if layout == 'oihw' else (KK, d.Cout * KK)
    return d


def _fields(d):
    return {n: getattr(d, n) for n, t in d._fields_ if n != 'reserved'}


def _answers(lib, family, d):
    return {name + ''.join('/%d' % a for a in extra): int(getattr(lib, name)(C.byref(d), *extra))
            for name, extra in FAMILIES[family][2]}


def _rows():
    for family in FAMILIES:
        for i, row in enumerate(TABLE[family]):
            yield '%s/%02d' % (family, i), family, row


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_and_the_golden_file_name_the_same_rows(golden):
    assert sorted(golden) == sorted(key for key, _, _ in _rows())
    assert len(golden) >= 40


@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_every_plan_answers_what_it_answered_before_the_helpers_were_shared(built_lib, golden, family):
    from iterative_inference_segm_amd import _lib
    lib = _lib.load()
    for key, fam, row in _rows():
        if fam != family:
            continue
        d = _desc(family, row)
        assert _fields(d) == golden[key]['desc'], key                   # the row still describes what was recorded
        assert _answers(lib, family, d) == golden[key]['answers'], (key, row)


def test_the_table_reaches_every_branch_the_helpers_decide(golden):
    for family in FAMILIES:
        rows = [v for k, v in golden.items() if k.startswith(family + '/')]
        slabs = [a for v in rows for n, a in v['answers'].items() if n.endswith('_slabs')]
        assert any(a == -2 for v in rows for a in v['answers'].values()), family     # a refusal
        assert any(a >= 0 for v in rows for a in v['answers'].values()), family
        if family != 'dgrad':                                                          # (no split there)
            assert 1 in slabs and any(a > 1 for a in slabs), family


if __name__ == '__main__' and '--record' in sys.argv:
    sys.path.insert(0, ROOT)
    from iterative_inference_segm_amd import _lib
    out = {}
    for key, family, row in _rows():
        d = _desc(family, row)
        out[key] = {'desc': _fields(d), 'answers': _answers(_lib.load(), family, d)}
    with open(GOLDEN, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print('recorded %d rows' % len(out))
