"""python -m nabu_amd.scripts.lm: estimate a label n-gram (processing/ngram_lm.py) from normalised transcriptions.

    python -m nabu_amd.scripts.lm --text FILE (--alphabet "a b c" | --datadir DIR) --order N --out lm.npz

--text lines are `<utterance id> <symbol> <symbol> ...`, the normalised form TextProcessor writes; --datadir reads
`alphabet` from a target directory written by `run data`.  A symbol outside the alphabet is an error naming the line.
The file is what the decoders' lm_file key takes."""
import argparse
import os

from nabu_amd.processing import ngram_lm


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--text', required=True, help='normalised transcriptions: <utterance id> <symbol> ...')
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--alphabet', help='space separated symbols')
    src.add_argument('--datadir', help='a target directory written by `run data` (its `alphabet` file)')
    ap.add_argument('--order', type=int, required=True)
    ap.add_argument('--out', required=True)
    args = ap.parse_args(argv)
    if args.datadir is not None:
        with open(os.path.join(args.datadir, 'alphabet')) as fid:
            alphabet = fid.read().strip().split(' ')
    else:
        alphabet = args.alphabet.strip().split(' ')
    ngram_lm.check_size(args.order, len(alphabet) + 1)
    sentences = ngram_lm.read_text(args.text, alphabet)
    lm = ngram_lm.train(sentences, alphabet, args.order)
    lm.save(args.out)
    print('%s: order %d over %d symbols + boundary from %d sentences, %d table entries'
          % (args.out, lm.order, len(alphabet), len(sentences), lm.logprobs.size))
    return lm


if __name__ == '__main__':
    main()
