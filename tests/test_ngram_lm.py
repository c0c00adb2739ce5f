"""CPU: the dense label n-gram (nabu_amd/processing/ngram_lm.py) against its independent restatement
(tests/ngram_lm_ref.py) and by hand; the model file, the loader's refusals and the command line."""
import numpy as np
import pytest

from nabu_amd.processing import ngram_lm as L
from tests import ngram_lm_ref as R

C = 4                                               # labels 0, 1, 2 and the boundary 3
CORPUS = [[0, 1], [0, 1, 2], [1]]                   # the three sentences of the hand-computed bigram
ALPHABET = ['a', 'b', 'c']


def random_corpus(seed, C, count=30):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, C - 1, rng.integers(0, 7)).tolist() for _ in range(count)]


@pytest.mark.parametrize('order', [1, 2, 3])
def test_rows_sum_to_one_entries_are_positive_and_the_restatement_agrees(order):
    for corpus, c in ((CORPUS, C), (random_corpus(order, 6), 6), ([], 3)):
        p = L.estimate(corpus, c, order)
        assert p.shape == (c ** (order - 1), c) and p.dtype == np.float64
        assert np.all(p > 0)
        np.testing.assert_allclose(p.sum(1), 1.0, rtol=0, atol=1e-12)
        np.testing.assert_allclose(p, R.table(corpus, c, order), rtol=1e-13, atol=0)


def test_bigram_by_hand():
    """CORPUS padded: 3 0 1 3 | 3 0 1 2 3 | 3 1 3.  Unigram counts: 0:2, 1:3, 2:1, 3(end):3, total 9, four distinct
    successors, p_0 = 1/4: p_1(c) = (count + 4/4) / (9 + 4)."""
    p1 = np.array([3, 4, 2, 4]) / 13.0
    np.testing.assert_allclose(L.estimate(CORPUS, C, 1)[0], p1, rtol=1e-15)
    p = L.estimate(CORPUS, C, 2)
    # after the start (row 3): 0 twice, 1 once -> count 3, two distinct successors
    np.testing.assert_allclose(p[3], (np.array([2, 1, 0, 0]) + 2 * p1) / 5.0, rtol=1e-15)
    # after 0: always 1 -> count 2, one distinct successor
    np.testing.assert_allclose(p[0], (np.array([0, 2, 0, 0]) + 1 * p1) / 3.0, rtol=1e-15)
    # after 1: end twice, 2 once
    np.testing.assert_allclose(p[1], (np.array([0, 0, 1, 2]) + 2 * p1) / 5.0, rtol=1e-15)
    # after 2: end once
    np.testing.assert_allclose(p[2], (np.array([0, 0, 0, 1]) + 1 * p1) / 2.0, rtol=1e-15)


def test_an_unseen_context_is_its_backed_off_row():
    p2, p3 = L.estimate(CORPUS, C, 2), L.estimate(CORPUS, C, 3)
    # (2, 0) never occurs: p_3(. | 2 0) = p_2(. | 0); index = oldest * C + most recent
    np.testing.assert_array_equal(p3[2 * C + 0], p2[0])
    # (0, 1) occurs: it is not simply the backed-off row
    assert not np.allclose(p3[0 * C + 1], p2[1])
    # a context nobody saw at any order ends at the unigram
    np.testing.assert_array_equal(L.estimate([[0]], C, 3)[2 * C + 2], L.estimate([[0]], C, 1)[0])


def test_context_indexing_next_and_the_boundary_padding():
    lm = L.train(CORPUS, ALPHABET, 3)
    assert lm.num_contexts == 16 and lm.start_context() == 15 == R.start_context(C, 3)     # both digits the boundary
    ctx = lm.start_context()
    for c, want in ((0, 3 * C + 0), (1, 0 * C + 1), (2, 1 * C + 2), (2, 2 * C + 2)):      # most recent least significant
        ctx = lm.next(ctx, c)
        assert ctx == want == R.context_index((want // C, want % C), C)
    one = L.train(CORPUS, ALPHABET, 1)
    assert one.num_contexts == 1 and one.start_context() == 0 and one.next(0, 2) == 0
    # padding: n-1 boundaries in front — the first label is predicted from the all-boundary row, which is seen —
    # and one at the end, predicted like a label
    p3 = L.estimate(CORPUS, C, 3)
    assert p3[15, 0] > p3[15, 1] > p3[15, 2] and p3[0 * C + 1, 3] > 0.25
    got = lm.sequence_logprob([0, 1])
    want = np.log(p3[15, 0]) + np.log(p3[3 * C + 0, 1]) + np.log(p3[0 * C + 1, 3])
    assert got == pytest.approx(want, rel=1e-6)
    assert got == pytest.approx(R.sequence_logprob(lm.logprobs.astype(np.float64), [0, 1], C, 3), rel=1e-12)


def test_npz_round_trip(tmp_path):
    lm = L.train(CORPUS, ALPHABET, 2)
    path = str(tmp_path / 'lm.npz')
    lm.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ['alphabet', 'logprobs', 'num_labels', 'order']
        assert z['logprobs'].dtype == np.float32 and z['logprobs'].shape == (4, 4)
    back = L.load(path, num_labels=4, alphabet=ALPHABET)
    assert (back.order, back.num_labels, back.alphabet) == (2, 4, ALPHABET)
    np.testing.assert_array_equal(back.logprobs, lm.logprobs)
    np.testing.assert_allclose(np.exp(back.logprobs.astype(np.float64)).sum(1), 1.0, atol=1e-6)


def test_the_loader_refuses(tmp_path):
    path = str(tmp_path / 'lm.npz')
    L.train(CORPUS, ALPHABET, 2).save(path)
    with pytest.raises(ValueError, match='num_labels is 4.*output dimension \\+ 1 = 6'):
        L.load(path, num_labels=6)
    with pytest.raises(ValueError, match='alphabet'):
        L.load(path, num_labels=4, alphabet=['a', 'c', 'b'])

    def write(**fields):
        base = dict(order=np.int64(2), num_labels=np.int64(4), logprobs=np.zeros((4, 4), np.float32),
                    alphabet=np.array(ALPHABET))
        base.update(fields)
        with open(path, 'wb') as fid:
            np.savez(fid, **base)
    write(order=np.int64(0))
    with pytest.raises(ValueError, match='order must be at least 1'):
        L.load(path)
    write(order=np.int64(5), num_labels=np.int64(41))                 # 41^5 > 2^24
    with pytest.raises(ValueError, match='2\\^24'):
        L.load(path)
    write(logprobs=np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match='shape'):
        L.load(path)
    with pytest.raises(ValueError, match='2\\^24'):
        L.estimate([], 64, 5)
    assert L.check_size(4, 64) == 64 ** 3                             # exactly 2^24 entries: the largest accepted


def test_command_line(tmp_path, capsys):
    from nabu_amd.scripts import lm as cli
    text = tmp_path / 'text'
    text.write_text('utt1 a b\nutt2 a b c\n\nutt3 b\n')
    out = str(tmp_path / 'lm.npz')
    cli.main(['--text', str(text), '--alphabet', 'a b c', '--order', '2', '--out', out])
    assert 'order 2' in capsys.readouterr().out
    got = L.load(out, 4, ALPHABET)
    np.testing.assert_array_equal(got.logprobs, L.train(CORPUS, ALPHABET, 2).logprobs)
    # --datadir: the alphabet file of a target directory
    (tmp_path / 'alphabet').write_text('a b c')
    out2 = str(tmp_path / 'lm2.npz')
    cli.main(['--text', str(text), '--datadir', str(tmp_path), '--order', '3', '--out', out2])
    assert L.load(out2).order == 3
    text.write_text('utt1 a b\nutt2 a x c\n')
    with pytest.raises(ValueError, match="line 2 \\(utt2\\): symbol 'x'"):
        cli.main(['--text', str(text), '--alphabet', 'a b c', '--order', '2', '--out', out])
    with pytest.raises(SystemExit):
        cli.main(['--text', str(text), '--order', '2', '--out', out])          # neither --alphabet nor --datadir
