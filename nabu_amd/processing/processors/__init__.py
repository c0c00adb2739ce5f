"""Processors turn one line of a data file (a wav path, a transcription) into what a writer stores: the
role of nabu/processing/processors in the reference.  `run data` (nabu_amd/scripts/data.py) drives them."""
