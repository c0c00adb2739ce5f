"""Writes tests/golden/features.npz: seeded int16 signals of about a second and the features the host
restatement (tests/feat_ref.py, float64) gives for them.  The file pins the restatement: a change of feat_ref
that moves these numbers is caught by tests/test_feature_processors.py.

    python tests/golden/make_features_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import feat_ref  # noqa: E402

CASES = {
    'fbank16k': (16000, 1.0, 11, dict()),
    'mfcc8k': (8000, 1.1, 12, dict(kind='mfcc', nfft=256)),
    'fbank16k_static': (16000, 0.9, 13, dict(dynamic='nodelta', include_energy=False, mvn=False)),
}


def main():
    out = {}
    for name, (rate, seconds, seed, conf) in CASES.items():
        sig = feat_ref.speech_like(seconds, rate, seed)
        out[name + '.signal'] = sig
        out[name + '.features'] = feat_ref.features(sig, rate, **conf)
    np.savez_compressed(os.path.join(HERE, 'features.npz'), **out)


if __name__ == '__main__':
    main()
