"""CPU: the four attention-dropout entry points are declared, exported and bound; their two new refusals and the plain
entry points' refusals fire with these functions' names; the `attention_dropout` key of both encoders.  No GPU needed."""
import ctypes
import os

import pytest

ONE = ctypes.c_void_p(16)     # any aligned non-null pointer: validation happens before it is touched


@pytest.mark.parametrize('what', ['fwd', 'bwd'])
@pytest.mark.parametrize('stem', ['self_attn_drop', 'self_attn_bf16_drop'])
def test_the_drop_entry_points_validate_on_the_host(stem, what):
    from nabu_amd import _hip
    lib, name = _hip.lib(), ('%s_%s: ' % (stem, what)).encode()
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'nabu_hip.h')) as fid:
        assert 'int nabu_%s_%s(' % (stem, what) in fid.read() and 'nabu_%s_%s' % (stem, what) in _hip.SIGNATURES

    def call(T=5, H=2, dk=64, ld=0, qkv=ONE, keep=0.9):
        rest = (ONE, keep, 1, 2, ONE, ONE) if what == 'fwd' else (ONE, ONE, ONE, ONE, keep, 1, 2, ONE)
        return getattr(lib, 'nabu_%s_%s' % (stem, what))(2, T, H, dk, qkv, ld or 3 * H * dk, *rest, None)
    for keep in (0.0, 1.5, float('nan'), -0.5, float('inf')):
        assert call(keep=keep) == -1 and name + b'keep = ' in lib.nabu_last_error() and b'(0, 1]' in lib.nabu_last_error()
    assert call(T=2 ** 20 + 1) == -1 and name + b'T = 1048577 > 2^20' in lib.nabu_last_error()
    assert call(dk=48) == -1 and name + b'head width dk = 48, must be 32 or 64' in lib.nabu_last_error()
    assert call(H=17) == -1 and b'1024' in lib.nabu_last_error()
    assert call(ld=380) == -1 and name + b'ld = 380 < 3 D = 384' in lib.nabu_last_error()
    assert call(ld=386) == -1 and b'multiple of 4' in lib.nabu_last_error()
    assert call(qkv=None) == -1 and name + b'null pointer' in lib.nabu_last_error()
    assert call(qkv=ctypes.c_void_p(20)) == -1 and name + b'qkv' in lib.nabu_last_error() and b'16-byte aligned' in lib.nabu_last_error()
    assert call(T=0) == 0 and call(T=0, keep=1.0) == 0                                   # nothing to do: no launch


@pytest.mark.parametrize('recipe', ['transformer_ctc', 'conformer_ctc'])
def test_the_attention_dropout_key(recipe):
    """refused at construction at 0, at 1.5 and when it is no number; 1.0 when absent, as in every shipped recipe"""
    from nabu_amd import recipes
    from nabu_amd.neuralnetworks.models.ed_encoders.transformer import attention_dropout_key
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    from nabu_amd.processing.synthetic import SyntheticData
    data = SyntheticData(3, 30, 15, min_frames=17, min_labels=1, max_labels=2, time_reduction=8, seed=7)

    def conf(**over):
        mc, tc, ec = recipes.load_recipe(recipe, **over)
        return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                                   server=None, task_index=0).model.encoder.conf
    for value in ('0', '1.5', 'half', 'nan'):
        with pytest.raises(ValueError, match='attention_dropout'):
            conf(**{'encoder.attention_dropout': value})
    assert 'attention_dropout' not in conf() and attention_dropout_key(conf()) == 1.0
    assert attention_dropout_key(conf(**{'encoder.attention_dropout': 0.8})) == 0.8
