"""CPU: host-side refusals of the bf16 self-attention entry points (self_attn_bf16.hip) with their messages, and the
`attention_precision` key of the transformer encoder; no GPU needed."""
import ctypes

import pytest


def test_self_attn_bf16_entry_points_validate_on_the_host():
    from nabu_amd import _hip, ops as hip
    lib = _hip.lib()
    one = ctypes.c_void_p(16)          # any aligned non-null pointer: validation happens before it is touched
    assert lib.nabu_self_attn_bf16_tile_q() % 32 == 0 and lib.nabu_self_attn_bf16_tile_k() % 32 == 0
    assert hip.self_attn_tiles('bf16') == (lib.nabu_self_attn_bf16_tile_q(), lib.nabu_self_attn_bf16_tile_k())

    fwd = lambda B=2, H=2, dk=64, ld=0, qkv=one, o=one: lib.nabu_self_attn_bf16_fwd(B, 5, H, dk, qkv, ld or 3 * H * dk, one, o, one, None)
    bwd = lambda B=2, H=2, dk=64, ld=0, do=one: lib.nabu_self_attn_bf16_bwd(B, 5, H, dk, one, ld or 3 * H * dk, one, one, do, one, one, None)
    for call, name in ((fwd, b'self_attn_bf16_fwd: '), (bwd, b'self_attn_bf16_bwd: ')):
        assert call(dk=48) == -1 and name + b'head width dk = 48, must be 32 or 64' in lib.nabu_last_error()
        assert call(H=17) == -1 and b'1024' in lib.nabu_last_error()            # D = 1088
        assert call(H=33, dk=32) == -1 and b'1024' in lib.nabu_last_error()
        assert call(ld=380) == -1 and name + b'ld = 380 < 3 D = 384' in lib.nabu_last_error()
        assert call(ld=386) == -1 and b'multiple of 4' in lib.nabu_last_error()
        assert call(B=65536) == -1 and name + b'B = 65536 > 65535' in lib.nabu_last_error()
    assert fwd(qkv=None) == -1 and b'self_attn_bf16_fwd: null pointer' in lib.nabu_last_error() and fwd(o=None) == -1
    assert bwd(do=None) == -1 and b'self_attn_bf16_bwd: null pointer' in lib.nabu_last_error()
    assert fwd(qkv=ctypes.c_void_p(20)) == -1 and b'self_attn_bf16_fwd: qkv and o must be 16-byte aligned' in lib.nabu_last_error()
    assert bwd(do=ctypes.c_void_p(20)) == -1 and b'self_attn_bf16_bwd: qkv, o, do and dqkv must be 16-byte' in lib.nabu_last_error()
    with pytest.raises(_hip.NabuHipError, match='precision'):
        hip.self_attn_tiles('f16')


def test_the_attention_precision_key():
    """refused at construction unless f32 or bf16; absent, it leaves layer.ATTENTION_PRECISION at f32 when encode sets up"""
    from nabu_amd import recipes, variables as vs
    from nabu_amd.neuralnetworks.components import layer
    from nabu_amd.neuralnetworks.trainers import trainer_factory
    from nabu_amd.processing.synthetic import SyntheticData
    data = SyntheticData(3, 30, 15, min_frames=17, min_labels=1, max_labels=2, time_reduction=8, seed=7)

    def trainer(**over):
        mc, tc, ec = recipes.load_recipe('transformer_ctc', **over)
        return trainer_factory.factory('standard')(conf=tc, dataconf=data, modelconf=mc, evaluatorconf=ec, expdir=None,
                                                   server=None, task_index=0)
    with pytest.raises(ValueError, match='attention_precision'):
        trainer(**{'encoder.attention_precision': 'fp8'})
    for value, want in (('bf16', 'bf16'), (None, 'f32')):
        tr = trainer(**({'encoder.attention_precision': value} if value else {}))
        with vs.as_default(tr.model.store):
            tr.model.encoder({}, {}, False)                              # no input: encode sets the precisions up, no more
        assert layer.ATTENTION_PRECISION[0] == want
