"""The `phones` normalizer (reference: nabu/processing/target_normalizers/phones.py): a phonetic
transcription already is a space separated symbol string."""


def normalize(transcription, _):
    return transcription
