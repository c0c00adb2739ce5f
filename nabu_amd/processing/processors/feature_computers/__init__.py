"""Feature computers: audio samples -> [frames, dim] features on the device (nabu_amd/csrc/features.hip)."""
