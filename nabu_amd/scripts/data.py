"""Data preparation entry point (reference: nabu/scripts/data.py:11-59): processes the data files of the
first section of <expdir>/database.conf with the processor of <expdir>/processor.cfg and writes the result
with the writer named by the section's `type`, then the processor's metadata.

    python -m nabu_amd.scripts.data --expdir DIR

Audio is not processed line by line: lines are collected until they hold MAX_BATCH_SAMPLES samples and a batch
goes to the device at once (inside a batch, utterances of one sample rate share the launches)."""
import argparse
import gzip
import os
from configparser import ConfigParser

from nabu_amd.processing.processors import processor_factory
from nabu_amd.processing.tfwriters import tfwriter_factory

# 16 Mi samples: about 17 minutes of 16 kHz audio, 32 MiB of int16 on the device and, at the default
# 123 columns every 160 samples, about 50 MiB of features
MAX_BATCH_SAMPLES = 1 << 24


def main(expdir):
    '''main function'''
    parsed_cfg = ConfigParser()
    parsed_cfg.read(os.path.join(expdir, 'database.conf'))
    conf = dict(parsed_cfg.items(parsed_cfg.sections()[0]))
    proc_cfg = ConfigParser()
    proc_cfg.read(os.path.join(expdir, 'processor.cfg'))
    processor = processor_factory.factory(proc_cfg.get('processor', 'processor'))(proc_cfg)
    writer = tfwriter_factory.factory(conf['type'])(conf['dir'])
    batched = hasattr(processor, 'process_loaded')
    names, loaded, held = [], [], 0

    def flush():
        for name, processed in zip(names, processor.process_loaded(loaded)):
            if processed is not None:
                writer.write(processed, name)
        del names[:], loaded[:]

    for datafile in conf['datafiles'].split(' '):
        open_fn = gzip.open if datafile.endswith('.gz') else open
        with open_fn(datafile, 'rt') as fid:
            for line in fid:
                splitline = line.strip().split(' ')
                name, dataline = splitline[0], ' '.join(splitline[1:])
                if not batched:
                    processed = processor(dataline)
                    if processed is not None:
                        writer.write(processed, name)
                    continue
                utt = processor.load(dataline)
                if loaded and held + len(utt[1]) > MAX_BATCH_SAMPLES:
                    flush()
                    held = 0
                names.append(name)
                loaded.append(utt)
                held += len(utt[1])
    if loaded:
        flush()
    processor.write_metadata(conf['dir'])


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--expdir', default='expdir', help='The experiments directory')
    main(ap.parse_args().expdir)
