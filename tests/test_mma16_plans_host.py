"""CPU: the plans behind the bf16 gradient / forward entry points (csrc/mma16_common.h: the parameter-layout check,
the slab split; csrc/conv_wgrad_common.h, conv_wgrad_kxk.hip, conv_dgrad_bf16.hip, conv_kxk_bf16.hip) return what
they returned before the shared helpers existed.  tests/golden/mma16_plans.json holds, for the table of descriptors
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
}

EDGES = (1, 63, 64, 65, 100)                       # around the 64-channel block, and a non-multiple of 16
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
                       dict(pad=100, H=4, W=4), dict(pad=0, H=2, W=9)],
    'dgrad': COMMON + [dict(pad=0), dict(accumulate=1), dict(accumulate=2), dict(Cin=512, Cout=512, H=422, W=422)],
    'kxk_wgrad': COMMON + KS + [dict(K=3, Cin=512, Cout=512, B=4, H=66, W=66), dict(K=3, Cin=1024, Cout=1024),
                                dict(K=1, H=37, W=150, B=3), dict(B=10, Cin=512, Cout=4096),
                                dict(B=10, Cin=4096, Cout=4096, K=1, H=1, W=1), dict(x_row=12), dict(x_y0=-1)],
    'kxk_dgrad': COMMON + KS + [dict(B=16, Cin=512, Cout=4096), dict(B=64, H=58, W=58, Cout=512),
                                dict(Cin=33, Cout=130), dict(accumulate=2), dict(K=1, H=37, W=150, B=3)],
    'kxk_fwd': [r for r in COMMON if not set(r) & {'layout', 'ci0', 'Cin_tot', 'so', 'sc'}] + KS +
               [dict(Cin=4096, Cout=4096), dict(B=16, H=70, W=70, Cout=256), dict(relu=2),
                dict(K=1, H=37, W=150, B=3, Cin=512, Cout=21)],
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
