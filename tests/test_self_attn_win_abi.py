"""CPU: the four chunk-window entry points are declared, exported and bound and refuse on the host; the cfg keys."""
import ctypes
import os

import pytest

ONE = ctypes.c_void_p(16)     # any aligned non-null pointer: validation happens before it is touched


@pytest.mark.parametrize('what', ['fwd', 'bwd'])
@pytest.mark.parametrize('stem', ['self_attn_win', 'self_attn_bf16_win'])
def test_the_win_entry_points_validate_on_the_host(stem, what):
    from nabu_amd import _hip
    lib, name = _hip.lib(), ('%s_%s: ' % (stem, what)).encode()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'nabu_hip.h')) as fid:
        assert 'int nabu_%s_%s(' % (stem, what) in fid.read() and 'nabu_%s_%s' % (stem, what) in _hip.SIGNATURES

    def call(T=5, H=2, dk=64, ld=0, qkv=ONE, keep=1.0, chunk=2, left=-1):
        rest = (ONE, keep, 1, 2, chunk, left, ONE, ONE) if what == 'fwd' else (ONE, ONE, ONE, ONE, keep, 1, 2, chunk, left, ONE)
        return getattr(lib, 'nabu_%s_%s' % (stem, what))(2, T, H, dk, qkv, ld or 3 * H * dk, *rest, None)
    for chunk in (0, -3):
        assert call(chunk=chunk) == -1 and name + b'chunk = %d, must be at least 1' % chunk in lib.nabu_last_error()
    assert call(left=-2) == -1 and name + b'left_chunks = -2, must be -1' in lib.nabu_last_error()
    for keep in (0.0, 1.5, float('nan')):
        assert call(keep=keep) == -1 and name + b'keep = ' in lib.nabu_last_error() and b'(0, 1]' in lib.nabu_last_error()
    assert call(T=2 ** 20 + 1) == -1 and name + b'T = 1048577 > 2^20' in lib.nabu_last_error()
    assert call(dk=48) == -1 and name + b'head width dk = 48, must be 32 or 64' in lib.nabu_last_error()
    assert call(H=17) == -1 and b'1024' in lib.nabu_last_error()
    assert call(ld=380) == -1 and name + b'ld = 380 < 3 D = 384' in lib.nabu_last_error()
    assert call(ld=386) == -1 and b'multiple of 4' in lib.nabu_last_error()
    assert call(qkv=None) == -1 and name + b'null pointer' in lib.nabu_last_error()
    assert call(qkv=ctypes.c_void_p(20)) == -1 and name + b'qkv' in lib.nabu_last_error() and b'16-byte aligned' in lib.nabu_last_error()
    assert call(T=0) == 0 and call(T=0, chunk=2 ** 31 - 1, left=2 ** 31 - 1) == 0        # nothing to do: no launch


@pytest.mark.parametrize('recipe', ['transformer_ctc', 'conformer_ctc'])
def test_the_attention_window_keys(recipe):
    """refused values, left chunks without a chunk, and the defaults when absent (as in every shipped recipe)"""
    from nabu_amd import recipes
    from nabu_amd.neuralnetworks.models.ed_encoders.transformer import attention_window_key
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    from nabu_amd.processing.synthetic import SyntheticData
    data = SyntheticData(3, 30, 15, min_frames=17, min_labels=1, max_labels=2, time_reduction=8, seed=7)

    def encoder(**over):
        mc, tc, ec = recipes.load_recipe(recipe, **{'encoder.' + k: v for k, v in over.items()})
        return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                                   server=None, task_index=0).model.encoder
    for value in ('0', '-1', '2.5', 'all'):
        with pytest.raises(ValueError, match='attention_chunk'):
            encoder(attention_chunk=value)
    for value in ('-2', '0.5', 'all'):
        with pytest.raises(ValueError, match='attention_left_chunks'):
            encoder(attention_chunk=4, attention_left_chunks=value)
    with pytest.raises(ValueError, match='attention_left_chunks'):
        encoder(attention_left_chunks=1)
    plain = encoder()
    assert 'attention_chunk' not in plain.conf and attention_window_key(plain.conf) is None and plain.attention_window is None
    assert encoder(attention_chunk=4).attention_window == (4, -1)
    assert encoder(attention_chunk=1, attention_left_chunks=0).attention_window == (1, 0)
