"""CPU: size query and host-side argument errors of the convolution entry points (conv2d.hip); no GPU needed."""
import ctypes


def test_conv_entry_points_validate_on_the_host():
    from nabu_amd import _hip
    lib = _hip.lib()
    one = ctypes.c_void_p(16)          # any aligned non-null pointer: validation happens before it is touched
    assert lib.nabu_conv_tile_t() >= 1
    per = (9 * 64 * 64 + 64) * 4
    assert lib.nabu_conv_ws_bytes(2, 5, 41, 64, 64) == per                  # 4 (b, time tile) pairs: one split
    ws = lib.nabu_conv_ws_bytes(32, 1000, 41, 64, 64)
    assert ws % per == 0 and 1 < ws // per <= 512
    assert lib.nabu_conv_ws_bytes(2, 5, 41, 64, 48) == 0 == lib.nabu_conv_ws_bytes(2, 5, 0, 64, 64)
    fwd = lambda F, Cout, x=one, w=one: lib.nabu_conv3x3_relu_fwd(2, 5, F, 3, Cout, x, None, one, w, one, 0, one, None)
    assert fwd(5, 48) == -1 and b'multiple of 32' in lib.nabu_last_error()
    assert fwd(0, 32) == -1 and b'F = 0' in lib.nabu_last_error()
    assert fwd(5, 32, x=None) == -1 and b'null pointer' in lib.nabu_last_error()
    bwd = lambda F, Cout, dw=one: lib.nabu_conv3x3_bwd_weights(2, 5, F, 3, Cout, one, one, one, one, dw, one, one, 1 << 30, None)
    assert bwd(5, 40) == -1 and bwd(0, 32) == -1 and bwd(5, 32, dw=None) == -1
    assert lib.nabu_conv3x3_bwd_weights(2, 5, 5, 3, 32, one, one, one, one, one, one, one, 16, None) == -3
    assert lib.nabu_maxpool2x2_fwd(2, 5, 0, 4, one, one, one, None) == -1 == lib.nabu_maxpool2x2_bwd(2, 5, 3, 4, one, one, None, one, None)
    assert lib.nabu_conv3x3_flip_weights(3, 32, None, one, None) == -1
