"""CPU: host-side refusals of the self-attention entry points (self_attn.hip), with their messages; no GPU needed."""
import ctypes


def test_self_attn_entry_points_validate_on_the_host():
    from nabu_amd import _hip
    lib = _hip.lib()
    one = ctypes.c_void_p(16)          # any aligned non-null pointer: validation happens before it is touched
    assert lib.nabu_self_attn_tile_q() % 32 == 0 and lib.nabu_self_attn_tile_k() % 32 == 0

    fwd = lambda H=2, dk=64, ld=0, qkv=one, o=one: lib.nabu_self_attn_fwd(2, 5, H, dk, qkv, ld or 3 * H * dk, one, o, one, None)
    bwd = lambda H=2, dk=64, ld=0, do=one: lib.nabu_self_attn_bwd(2, 5, H, dk, one, ld or 3 * H * dk, one, one, do, one, one, None)
    for call in (fwd, bwd):
        assert call(dk=48) == -1 and b'dk = 48, must be 32 or 64' in lib.nabu_last_error()
        assert call(H=17) == -1 and b'1024' in lib.nabu_last_error()            # D = 1088
        assert call(H=33, dk=32) == -1 and b'1024' in lib.nabu_last_error()
        assert call(ld=380) == -1 and b'ld = 380 < 3 D = 384' in lib.nabu_last_error()
        assert call(ld=386) == -1 and b'multiple of 4' in lib.nabu_last_error()
    assert fwd(qkv=None) == -1 and b'self_attn_fwd: null pointer' in lib.nabu_last_error() and fwd(o=None) == -1
    assert bwd(do=None) == -1 and b'self_attn_bwd: null pointer' in lib.nabu_last_error()
    assert fwd(qkv=ctypes.c_void_p(20)) == -1 and b'16-byte aligned' in lib.nabu_last_error()
    assert lib.nabu_add_positions_f32(2, 5, 8, None, one, one, None) == -1 and b'null pointer' in lib.nabu_last_error()
