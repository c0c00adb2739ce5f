"""Target normalizers: transcription string -> space separated symbols of the alphabet
(the role of nabu/processing/target_normalizers)."""
