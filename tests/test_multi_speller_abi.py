"""CPU tests of the C ABI of the Speller over several encoded inputs (include/nabu_hip.h, nabu_speller_multi_*):
exported symbols, ctypes struct sizes against the header's layout, host-side size queries and argument errors."""
import ctypes

from nabu_amd import _hip


def _desc(M, B, U, C, L, nl, Tes, Es, kind=0, K=0, F=0, prob_fn=0):
    i4 = ctypes.c_int32 * _hip.SPELLER_MAX_MEMORIES
    pad = [0] * (_hip.SPELLER_MAX_MEMORIES - len(Tes))
    return _hip.SpellerMultiDesc(ctypes.sizeof(_hip.SpellerMultiDesc), M, B, U, C, L, nl, i4(*(list(Tes) + pad)),
                                 i4(*(list(Es) + pad)), kind, K, F, prob_fn, 1.0, 0, 0, 0.0, 0, 0)


def test_symbols_and_struct_sizes():
    from nabu_amd import build
    build.build(verbose=False)
    lib = _hip.lib()
    for n in ('reserve_bytes', 'ws_bytes', 'uses_persistent', 'attn_slices', 'fwd', 'bwd', 'decoder_inputs',
              'beam_ws_bytes', 'beam_search'):
        assert hasattr(lib, 'nabu_speller_multi_' + n)
        assert 'nabu_speller_multi_' + n in _hip.SIGNATURES
    assert _hip.SPELLER_MAX_MEMORIES == 4
    # uint32 size + 6 int32 + 2 x 4 int32 + 4 int32 = 76 bytes, float at 76, then 8-byte alignment:
    # 80 seed, 88 seed_offset, 96 sample_prob (+4 pad), 104 sample_seed, 112 sample_offset -> 120
    assert ctypes.sizeof(_hip.SpellerMultiDesc) == 120
    assert _hip.SpellerMultiDesc.keep_prob.offset == 76 and _hip.SpellerMultiDesc.sample_offset.offset == 112
    # uint32 + 5 int32 + 2 x 4 int32 + 6 int32 + 2 float = 88 bytes
    assert ctypes.sizeof(_hip.MultiBeamDesc) == 88
    assert ctypes.sizeof(_hip.SpellerMultiPtrs) == 8 * (5 * 4 + 2 + 2 * _hip.SPELLER_MAX_LAYERS)


def test_size_queries_and_refusals():
    from nabu_amd import build
    build.build(verbose=False)
    lib = _hip.lib()
    d = _desc(2, 3, 16, 6, 5, 2, (7, 12), (8, 24))
    res = lib.nabu_speller_multi_reserve_bytes(ctypes.byref(d))
    assert res > 0 and lib.nabu_speller_multi_ws_bytes(ctypes.byref(d)) > 0
    # the reserve grows with the second memory: keys, alignments and the wider context rows
    one = _desc(1, 3, 16, 6, 5, 2, (7,), (8,))
    assert 0 < lib.nabu_speller_multi_reserve_bytes(ctypes.byref(one)) < res
    assert lib.nabu_speller_multi_uses_persistent(ctypes.byref(d), 0) == 0
    assert lib.nabu_speller_multi_uses_persistent(ctypes.byref(d), 1) == 0
    assert [lib.nabu_speller_multi_attn_slices(ctypes.byref(d), m) for m in range(2)] == [1, 1]
    big = _desc(2, 32, 32, 6, 6, 1, (40, 64), (64, 32))
    assert [lib.nabu_speller_multi_attn_slices(ctypes.byref(big), m) for m in range(2)] == [3, 4]
    # reserve_bytes == 0 + nabu_last_error: the "unsupported shape" answer
    for bad, text in ((_desc(5, 3, 16, 6, 5, 2, (7, 12), (8, 24)), b'encoded inputs'),
                      (_desc(0, 3, 16, 6, 5, 2, (7, 12), (8, 24)), b'encoded inputs'),
                      (_desc(2, 3, 16, 6, 5, 2, (7, 12), (8, 22)), b'multiples of 4'),
                      (_desc(2, 3, 16, 6, 5, 9, (7, 12), (8, 24)), b'layers'),
                      (_desc(2, 3, 16, 6, 5, 2, (7, 0), (8, 24)), b'bad dimensions'),
                      (_desc(2, 3, 16, 6, 5, 2, (7, 12), (8, 24), prob_fn=3), b'probability_fn')):
        assert lib.nabu_speller_multi_reserve_bytes(ctypes.byref(bad)) == 0
        assert text in lib.nabu_last_error(), lib.nabu_last_error()
    short = _desc(2, 3, 16, 6, 5, 2, (7, 12), (8, 24))
    short.size = 8
    assert lib.nabu_speller_multi_reserve_bytes(ctypes.byref(short)) == 0 and b'descriptor size' in lib.nabu_last_error()
    # null pointers and a short workspace are refused before any launch
    one_p = ctypes.c_void_p(16)
    assert lib.nabu_speller_multi_fwd(ctypes.byref(d), None, one_p, one_p, one_p, one_p, one_p, one_p, one_p, 1 << 40, None) == -1


def test_multi_beam_search_validates_on_the_host():
    from nabu_amd import build
    build.build(verbose=False)
    lib = _hip.lib()
    i4 = ctypes.c_int32 * _hip.SPELLER_MAX_MEMORIES
    d = _hip.MultiBeamDesc(ctypes.sizeof(_hip.MultiBeamDesc), 2, 2, 16, 5, 1, i4(6, 9, 0, 0), i4(8, 12, 0, 0), 0, 0, 0, 0, 3, 4,
                           0.0, 1.0)
    assert lib.nabu_speller_multi_beam_ws_bytes(ctypes.byref(d)) > 0
    d.temperature = 0.0
    assert lib.nabu_speller_multi_beam_ws_bytes(ctypes.byref(d)) == 0 and b'temperature' in lib.nabu_last_error()
    d.temperature, d.M = 1.0, 5
    assert lib.nabu_speller_multi_beam_ws_bytes(ctypes.byref(d)) == 0 and b'encoded inputs' in lib.nabu_last_error()
