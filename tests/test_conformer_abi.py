"""CPU: host-side refusals of the convolution-module entry points (conv_module.hip), with their messages, and the
construction refusals of `encoder = conformer`; no GPU needed."""
import ctypes

import pytest


def test_conv_module_entry_points_validate_on_the_host():
    from nabu_amd import _hip
    lib = _hip.lib()
    one = ctypes.c_void_p(16)          # any aligned non-null pointer: validation happens before it is touched
    assert lib.nabu_conv_module_tile_t() > 0 and lib.nabu_conv_module_parts(3, 2 * lib.nabu_conv_module_tile_t() + 1) == 9

    def fwd(D=64, K=15, ld=0, u=one, y=one):
        return lib.nabu_conv_module_fwd(2, 5, D, K, u, ld or 2 * D, one, one, one, one, one, 1e-5, y, one, one, None)

    def bwd(D=64, K=15, ld=0, u=one, y=one):
        return lib.nabu_conv_module_bwd(2, 5, D, K, u, ld or 2 * D, *([one] * 8 + [y] + [one] * 3), None)
    for call, name in ((fwd, b'conv_module_fwd'), (bwd, b'conv_module_bwd')):
        for D in (0, 96, 1088):
            assert call(D=D) == -1 and b'D = %d, must be a multiple of 64' % D in lib.nabu_last_error()
        for K in (1, 4, 33):
            assert call(K=K) == -1 and b'K = %d, must be odd in 3..31' % K in lib.nabu_last_error()
        assert call(ld=124) == -1 and b'ld = 124 < 2 D = 128' in lib.nabu_last_error()
        assert call(ld=130) == -1 and b'multiple of 4' in lib.nabu_last_error()
        assert call(u=ctypes.c_void_p(20)) == -1 and b'16-byte aligned' in lib.nabu_last_error()
        assert call(u=None) == -1 and name + b': null pointer' in lib.nabu_last_error()
        assert call(y=None) == -1 and name + b': null pointer' in lib.nabu_last_error()
    assert lib.nabu_swish_f32(4, None, one, None) == -1 and b'swish: null pointer' in lib.nabu_last_error()
    assert lib.nabu_swish_bwd_f32(4, one, None, one, None) == -1 and b'swish_bwd: null pointer' in lib.nabu_last_error()


def test_the_recipe_resolves_and_the_encoder_refuses_bad_keys():
    from nabu_amd import recipes
    from nabu_amd.neuralnetworks.models.ed_encoders import conformer, ed_encoder_factory
    from nabu_amd.neuralnetworks.models.ed_decoders import ed_decoder_factory
    mc, tc, ec = recipes.load_recipe('conformer_ctc')
    cls = ed_encoder_factory.factory(mc.get('encoder', 'encoder'))
    assert cls is conformer.Conformer and ed_decoder_factory.factory(mc.get('decoder', 'decoder')) is not None
    assert cls(mc, None).conf['conv_kernel'] == '15'
    for key, value in (('conv_kernel', 4), ('conv_kernel', 33), ('num_units', 96), ('layer_norm', 'True')):
        with pytest.raises(ValueError, match=key):
            cls(recipes.load_recipe('conformer_ctc', **{'encoder.' + key: value})[0], None)
    mc.remove_option('encoder', 'conv_kernel')
    with pytest.raises(ValueError, match='conv_kernel'):
        cls(mc, None)
