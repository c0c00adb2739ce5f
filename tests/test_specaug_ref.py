"""CPU tests of SpecAugment: the host reference's rules (tests/specaug_ref.py), the cfg keys and their parser, the
DNN encoder's refusal, and the presence and host-side argument checks of the C entry point.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from nabu_amd import recipes
from tests import specaug_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAMS = [(7, 3), ((5 << 32) | 9, (3 << 32) | 1000003), ((1 << 40) + 3, (1 << 32) - 1)]


def test_every_draw_is_in_bounds():
    rng = np.random.default_rng(0)
    for trial in range(600):
        n, W = int(rng.integers(0, 60)), int(rng.integers(0, 8))
        Tw, Fw, blocks = int(rng.integers(0, 70)), int(rng.integers(0, 50)), int(rng.choice([1, 3]))
        ratio = float(rng.choice([0.05, 0.2, 1.0]))
        dblk = int(rng.integers(1, 42))
        pol = R.Policy(W, 2, Tw, ratio, 2, Fw, blocks)
        seed, offset = STREAMS[trial % 3]
        (c, cp), tm, fm = R.draw(trial % 6, n, dblk * blocks, pol, seed, offset + trial)
        if W > 0 and n >= 2 * W + 3:
            assert W + 1 <= c <= n - W - 2 and abs(cp - c) <= W and 1 <= cp <= n - 2, (n, W, c, cp)
        else:
            assert (c, cp) == (0, 0)
        cap = min(Tw, int(np.float32(ratio) * np.float32(n)))
        for t0, t in tm:
            assert 0 <= t <= cap <= n and 0 <= t0 and t0 + t <= n, (n, Tw, ratio, t0, t)
        for f0, f in fm:
            assert 0 <= f <= min(Fw, dblk) and 0 <= f0 and f0 + f <= dblk, (dblk, Fw, f0, f)


def test_warp_maps_the_anchor_frames_exactly_and_is_monotone():
    rng = np.random.default_rng(1)
    warped = 0
    for trial in range(1500):
        n, W = int(rng.integers(1, 60)), int(rng.integers(0, 8))
        (c, cp), _, _ = R.draw(trial % 7, n, 40, R.Policy(W, 0, 0, 1.0, 0, 0, 1), (5 << 32) | 9, (3 << 32) | trial)
        if n < 2 * W + 3 or W == 0:
            assert (c, cp) == (0, 0)                # too short for an anchor with W frames of room on both sides
            continue
        warped += 1
        assert R.warp_source(0, n, c, cp)[:2] == (0, 0)
        assert R.warp_source(cp, n, c, cp)[:2] == (c, 0)
        assert R.warp_source(n - 1, n, c, cp)[:2] == (n - 1, 0)
        pi, pr, pd = -1, 0, 1
        for t in range(n):
            i, r, d = R.warp_source(t, n, c, cp)
            assert 0 <= i <= n - 1 and 0 <= r < d and (i < n - 1 or r == 0), (t, n, c, cp, i, r)   # i + 1 read only if r > 0
            assert (i * d + r) * pd >= (pi * pd + pr) * d, (t, n, c, cp)                       # position i + r / d grows
            pi, pr, pd = i, r, d
    assert warped > 300


def test_smallest_warped_length():
    """n = 2 W + 3: the anchor can only be the middle frame W + 1; one frame less is not warped"""
    for W in (1, 5):
        n = 2 * W + 3
        seen = set()
        for b in range(40):
            (c, cp), _, _ = R.draw(b, n, 40, R.Policy(W, 0, 0, 1.0, 0, 0, 1), 7, 3)
            assert c == W + 1 and 1 <= cp <= 2 * W + 1
            seen.add(cp)
            assert R.draw(b, n - 1, 40, R.Policy(W, 0, 0, 1.0, 0, 0, 1), 7, 3)[0] == (0, 0)
        assert len(seen) > 1


def test_widths_reach_zero_and_their_cap_and_masks_may_overlap():
    pol = R.Policy(0, 2, 6, 1.0, 2, 4, 1)
    ts, fs, overlap = set(), set(), 0
    for b in range(400):
        _, tm, fm = R.draw(b, 30, 12, pol, 11, 5)
        ts.update(t for _, t in tm)
        fs.update(f for _, f in fm)
        (a0, a), (b0, bw) = tm
        overlap += a > 0 and bw > 0 and a0 < b0 + bw and b0 < a0 + a
    assert ts == set(range(7)) and fs == set(range(5))
    assert overlap > 0
    # the ratio caps a width below time_mask_width, the block width caps a frequency mask below freq_mask_width
    ts = {t for b in range(300) for _, t in R.draw(b, 30, 12, R.Policy(0, 2, 100, 0.2, 2, 100, 3), 11, 5)[1]}
    fs = {f for b in range(300) for _, f in R.draw(b, 30, 12, R.Policy(0, 2, 100, 0.2, 2, 100, 3), 11, 5)[2]}
    assert ts == set(range(7)) and fs == set(range(5))


def test_overlapping_masks_zero_their_union_and_padding_is_copied():
    pol = R.Policy(0, 2, 6, 1.0, 2, 4, 3)
    rng = np.random.default_rng(2)
    x = (rng.normal(size=(3, 20, 12)) + 3).astype(np.float32)          # no zero among the inputs
    lens = np.array([20, 13, 1])
    y, prm, frac, _ = R.augment(x, lens, pol, 11, 5)
    assert prm.shape == (3, 10) and not frac.any()
    for b in range(3):
        _, tm, fm = R.draw(b, int(lens[b]), 12, pol, 11, 5)
        rows = np.zeros(20, bool)
        for t0, t in tm:
            rows[t0:t0 + t] = True
        cols = np.zeros(4, bool)
        for f0, f in fm:
            cols[f0:f0 + f] = True
        zero = rows[:, None] | (np.tile(cols, 3)[None, :] & (np.arange(20) < lens[b])[:, None])
        np.testing.assert_array_equal(y[b] == 0, zero)
        np.testing.assert_array_equal(y[b][~zero], x[b][~zero])


def test_streams_differ():
    pol = R.Policy(3, 2, 10, 1.0, 2, 10, 1)
    lens = [37] * 6
    seen = [R.params(lens, 40, pol, s, o).tobytes() for s, o in STREAMS + [(7, 4), (8, 3), (7, 3 + (1 << 32)),
                                                                          (7 + (1 << 32), 3)]]
    assert len(set(seen)) == len(seen)
    p = R.params(lens, 40, pol, 7, 3)
    assert len({p[b].tobytes() for b in range(6)}) == 6           # and so do the utterances of one call


# ------------------------------------------------------------------------------------------------- cfg keys

def test_cfg_keys_default_to_off_and_parse():
    from nabu_amd.neuralnetworks.models.ed_encoders.listener import spec_augment_keys, SPEC_AUGMENT_KEYS
    off = spec_augment_keys({})
    assert not off.on and tuple(off) == (0, 0, 0, 1.0, 0, 0, 1) and off.param_width == 2
    over = {'encoder.time_warp': 80, 'encoder.time_masks': 2, 'encoder.time_mask_width': 100,
            'encoder.freq_masks': 2, 'encoder.freq_mask_width': 27, 'encoder.time_mask_ratio': 0.2,
            'encoder.feature_blocks': 3}
    assert sorted(k.split('.')[1] for k in over) == sorted(SPEC_AUGMENT_KEYS)
    for recipe in ('cfg2_listener_ctc', 'cfg1_dblstm_ctc', 'cfg3_las_vanilla'):
        mc, _, _ = recipes.load_recipe(recipe, **over)
        pol = spec_augment_keys(dict(mc.items('encoder')))
        assert pol.on and tuple(pol) == (80, 2, 100, 0.2, 2, 27, 3) and pol.param_width == 10
    assert spec_augment_keys({'freq_masks': '1'}).on and spec_augment_keys({'time_masks': '1'}).on
    assert not spec_augment_keys({'time_mask_width': '5', 'freq_mask_width': '5', 'feature_blocks': '3'}).on


@pytest.mark.parametrize('key,value', [
    ('time_warp', '-1'), ('time_warp', '2.5'), ('time_warp', str(1 << 24)), ('time_masks', '-1'), ('time_masks', '9'),
    ('time_masks', 'two'), ('time_mask_width', '-3'), ('time_mask_ratio', '0'), ('time_mask_ratio', '1.5'),
    ('time_mask_ratio', '-0.2'), ('time_mask_ratio', 'half'), ('time_mask_ratio', 'nan'), ('freq_masks', '-1'),
    ('freq_masks', '9'), ('freq_mask_width', '-1'), ('freq_mask_width', 'x'), ('feature_blocks', '0'),
    ('feature_blocks', '-3')])
def test_cfg_key_parser_raises_naming_the_key(key, value):
    from nabu_amd.neuralnetworks.models.ed_encoders.listener import spec_augment_keys
    with pytest.raises(ValueError, match=key):
        spec_augment_keys({key: value})


def test_feature_blocks_must_divide_the_feature_dimension():
    import torch
    from nabu_amd import ops as hip
    from nabu_amd.neuralnetworks.components import ops as nops
    rs = nops.RngState(1)
    with pytest.raises(ValueError, match='feature_blocks'):
        nops.spec_augment(torch.zeros(2, 5, 40), np.array([5, 3], np.int32), hip.SpecAugmentPolicy(freq_masks=1,
                          freq_mask_width=3, feature_blocks=3), rs)
    assert rs.offset == 0


def test_no_shipped_recipe_or_defaults_file_sets_a_key():
    from nabu_amd.neuralnetworks.models.ed_encoders.listener import spec_augment_keys, SPEC_AUGMENT_KEYS
    for recipe in sorted(os.listdir(recipes.RECIPES)):
        if not os.path.isdir(os.path.join(recipes.RECIPES, recipe)):
            continue
        mc, _, _ = recipes.load_recipe(recipe)
        conf = dict(mc.items('encoder'))
        assert not [k for k in SPEC_AUGMENT_KEYS if k in conf], recipe
        assert not spec_augment_keys(conf).on
    d = os.path.join(ROOT, 'nabu_amd', 'neuralnetworks', 'models', 'ed_encoders', 'defaults')
    for name in os.listdir(d):
        text = open(os.path.join(d, name)).read()
        assert not [k for k in SPEC_AUGMENT_KEYS if re.search(r'^\s*%s\s*=' % k, text, flags=re.M)], name


def test_a_policy_that_is_off_makes_no_call_and_takes_no_offset(monkeypatch):
    import torch
    from nabu_amd import ops as hip
    from nabu_amd.neuralnetworks.components import ops as nops
    from nabu_amd.neuralnetworks.models.ed_encoders import listener
    monkeypatch.setattr(hip, 'spec_augment', lambda *a, **k: pytest.fail('called'))
    rs = nops.RngState(5)
    x = torch.zeros(2, 4, 3)
    assert nops.spec_augment(x, np.array([4, 2]), hip.SpecAugmentPolicy(time_mask_width=9), rs) is x
    assert rs.offset == 0
    monkeypatch.setattr(nops, '_rng', rs)
    conf = {'input_noise': '0', 'time_mask_width': '5'}
    y, lens = listener.augment(conf, x, 'lengths', True)
    assert y is x and lens == 'lengths' and rs.offset == 0
    # not training: nothing either, whatever the keys say (and the keys are still validated)
    conf = {'input_noise': '0.6', 'time_warp': '2', 'time_masks': '2', 'time_mask_width': '5'}
    y, lens = listener.augment(conf, x, 'lengths', False)
    assert y is x and rs.offset == 0
    with pytest.raises(ValueError, match='time_masks'):
        listener.augment(dict(conf, time_masks='12'), x, 'lengths', False)


def test_dnn_encoder_refuses_the_keys():
    from nabu_amd.neuralnetworks.models.ed_encoders import ed_encoder_factory
    mc, _, _ = recipes.load_recipe('dnn_hybrid_wsj')
    ed_encoder_factory.factory('dnn')(mc, None)                      # the recipe as shipped builds
    for key, value in (('time_warp', 5), ('freq_masks', 2), ('feature_blocks', 3), ('time_mask_ratio', 0.2)):
        mc, _, _ = recipes.load_recipe('dnn_hybrid_wsj', **{'encoder.' + key: value})
        with pytest.raises(Exception, match='SpecAugment.*%s|%s.*SpecAugment' % (key, key)):
            ed_encoder_factory.factory('dnn')(mc, None)


# ------------------------------------------------------------------------------------------------- C ABI

def test_symbol_declared_bound_and_wrapped():
    from nabu_amd import _hip, ops, build
    from nabu_amd.neuralnetworks.components import ops as nops
    hdr = open(os.path.join(ROOT, 'include', 'nabu_hip.h')).read()
    assert re.search(r'\bnabu_spec_augment_f32\s*\(', hdr) and 'nabu_spec_augment_f32' in _hip.SIGNATURES
    assert callable(ops.spec_augment) and callable(nops.spec_augment)
    assert ops.SpecAugmentPolicy().param_width == 2
    build.build(verbose=False)
    assert hasattr(_hip.lib(), 'nabu_spec_augment_f32')
    # the descriptor's layout as the header declares it: eleven 4-byte fields
    assert ctypes.sizeof(_hip.SpecAugDesc) == 44
    fields = re.search(r'typedef struct nabu_specaug_desc \{(.*?)\}', hdr, flags=re.S).group(1)
    fields = re.sub(r'/\*.*?\*/', '', fields, flags=re.S)
    names = [n.strip() for decl in fields.split(';') if decl.strip() for n in decl.split(None, 1)[1].split(',')]
    assert names == [f[0] for f in _hip.SpecAugDesc._fields_]


def _desc(**kw):
    from nabu_amd import _hip
    v = dict(B=2, T=10, D=12, feature_blocks=1, time_warp=1, time_masks=1, time_mask_width=2, freq_masks=1,
             freq_mask_width=2, time_mask_ratio=1.0)
    v.update(kw)
    return _hip.SpecAugDesc(ctypes.sizeof(_hip.SpecAugDesc), v['B'], v['T'], v['D'], v['feature_blocks'], v['time_warp'],
                            v['time_masks'], v['time_mask_width'], v['freq_masks'], v['freq_mask_width'],
                            v['time_mask_ratio'])


@pytest.mark.parametrize('change,code,text', [
    (dict(T=1 << 24), -2, b'2^24'), (dict(T=(1 << 24) - 1, D=256), -2, b'T * D'), (dict(B=70000), -2, b'B = 70000'),
    (dict(B=-1), -1, b'negative'), (dict(time_warp=-1), -1, b'time_warp'), (dict(time_warp=1 << 24), -1, b'time_warp'),
    (dict(time_masks=9), -1, b'time_masks'), (dict(freq_masks=-1), -1, b'freq_masks'),
    (dict(freq_masks=9), -1, b'freq_masks'), (dict(time_mask_width=-1), -1, b'width'),
    (dict(freq_mask_width=-2), -1, b'width'), (dict(time_mask_ratio=0.0), -1, b'time_mask_ratio'),
    (dict(time_mask_ratio=1.25), -1, b'time_mask_ratio'), (dict(time_mask_ratio=float('nan')), -1, b'time_mask_ratio'),
    (dict(feature_blocks=0), -1, b'feature_blocks'), (dict(feature_blocks=5), -1, b'feature_blocks')])
def test_entry_point_validates_on_the_host(change, code, text):
    """every refusal comes before the launch: the pointers are never touched"""
    from nabu_amd import _hip, build
    build.build(verbose=False)
    lib = _hip.lib()
    x, y, ln = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10000 + (1 << 40)), ctypes.c_void_p(0x100)
    d = _desc(**change)
    assert lib.nabu_spec_augment_f32(ctypes.byref(d), x, ln, y, None, 1, 2, None) == code
    assert text in lib.nabu_last_error(), lib.nabu_last_error()


def test_entry_point_refuses_pointers_it_cannot_use():
    from nabu_amd import _hip, build
    build.build(verbose=False)
    lib = _hip.lib()
    d = _desc()
    x, y, ln = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x100)
    for args, text in (((None, ln, y), b'null'), ((x, None, y), b'null'), ((x, ln, None), b'null'),
                       ((x, ln, x), b'overlap'), ((x, ln, ctypes.c_void_p(0x10000 + 4 * 239)), b'overlap'),
                       ((x, ln, ctypes.c_void_p(0x20002)), b'aligned')):
        assert lib.nabu_spec_augment_f32(ctypes.byref(d), args[0], args[1], args[2], None, 1, 2, None) == -1
        assert text in lib.nabu_last_error(), (args, lib.nabu_last_error())
    short = _desc()
    short.size = 40
    assert lib.nabu_spec_augment_f32(ctypes.byref(short), x, ln, y, None, 1, 2, None) == -1
    # nothing to do is not an error (and launches nothing)
    assert lib.nabu_spec_augment_f32(ctypes.byref(_desc(B=0)), None, None, None, None, 1, 2, None) == 0
