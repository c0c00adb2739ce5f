"""Neural network trainer environment (reference:
nabu/neuralnetworks/trainers/trainer.py:18-792).

Same constructor arguments, same ``[trainer]`` cfg keys and defaults, same training
loop (read a batch -> update -> print -> increment the global step).  What changed
underneath:
  * the TF graph of one step is a sequence of HIP kernel launches on one stream
    (model forward, fused loss+gradient, hand-written backward kernels);
  * ``tf.train.AdamOptimizer`` + per-variable ``clip_by_value`` (trainer.py:525,
    560-569) is ONE fused clip+Adam kernel over a flat parameter buffer;
  * the parameter-server data parallelism (trainer.py:479-510, 822-914) is one
    RCCL all-reduce of the flat gradient buffer per step: every replica clips its
    own gradient, the clipped gradients are averaged, one Adam update is applied —
    the synchronous semantics the reference's SyncReplicasOptimizer branch
    intends with numbatches_to_aggregate = number of workers.
    ``numbatches_to_aggregate = A * replicas`` with A > 1 accumulates gradients on
    the device: every replica takes A batches per update, clips each one's gradient
    as a replica's is clipped before the exchange, sums them in a second flat
    buffer (nabu_clip_accumulate_f32), exchanges the local sum once and applies one
    Adam step on the mean of all A * replicas clipped gradients — the update
    A * replicas replicas make, on the batches they would read (step_accumulated;
    DESIGN.md section 6).  0 (the default) and ``replicas`` itself are the plain
    step; any other value is an error, the stale-gradient dropping of a
    SyncReplicasOptimizer that aggregates fewer gradients than it has workers is
    not reproduced.  Optional
    (``allreduce_buckets = True``, an extension key; default False): the same sum
    exchanged as one bucket per encoder layer (+ one for the decoder), each started
    as soon as its gradients are final and overlapped with the dense products of the
    next layer's backward pass — never with a persistent recurrent kernel;
  * ``clip_gradient_norm = c`` (an extension key; off when absent or 0) replaces the element clip by global-norm
    clipping after the aggregation: the mean of the update's A * replicas unclipped gradients times min(1, c / norm),
    the norm reduced on the device (nabu_grad_norm_f32) and the factor read there by the Adam launch
    (nabu_adam_scaled_step); an update whose norm is NaN or inf is skipped on the device;
  * ``mwer_nbest = N`` (an extension key with ``mwer_max_steps``, ``mwer_ce_weight``, ``mwer_start_step``; off when absent
    or 0) replaces the forward pass and the loss of a step by minimum word error rate training over the N-best list of
    the model's own beam search (trainers/mwer.py); everything behind the loss is the same;
  * ``train()`` is ONE loop around ``step`` / ``step_accumulated`` (one body, ``_run_update``, and one ``_update`` for
    every A and every exchange).  Two small objects say where a device batch comes from (DirectFeed | AheadFeed) and
    when a step's words are read (readback.ReadNow | ReadLate); ``prefetch_batches`` >= 1 (an extension key,
    DESIGN.md section 8) selects the second of each."""
import math
import sys
import os
import pickle
import time
from abc import ABCMeta, abstractmethod

import numpy as np
import torch

from nabu_amd import ops as hip
from nabu_amd.autodiff import Tape, SeqLen
from nabu_amd.neuralnetworks.models.model import Model
from nabu_amd.neuralnetworks.trainers import loss_functions, mwer, readback
from nabu_amd.tools.default_conf import apply_defaults, defaults_path

ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8      # tf.train.AdamOptimizer defaults
CLIP = 1.0                                         # tf.clip_by_value(grad, -1., 1.)
CHECKPOINT_SECS = 600                              # MonitoredTrainingSession default


def weight_noise_keys(conf):
    """the `weight_noise` and `weight_noise_start_step` keys of the [trainer] section (build additions like
    label_smoothing: absent from defaults/standardtrainer.cfg, 0 when absent) -> (stddev, start_step).  A step is noisy
    when stddev > 0 and global_step >= start_step."""
    text = str(conf.get('weight_noise', '0')).strip()
    try:
        stddev = float(text)
    except ValueError:
        raise ValueError('weight_noise must be a number, got %r' % text)
    if not (0.0 <= stddev < float('inf')):                      # (false for NaN)
        raise ValueError('weight_noise must be a finite standard deviation >= 0, got %r' % text)
    text = str(conf.get('weight_noise_start_step', '0')).strip()
    try:
        start = int(text)
    except ValueError:
        raise ValueError('weight_noise_start_step must be an integer, got %r' % text)
    if start < 0:
        raise ValueError('weight_noise_start_step must be >= 0, got %r' % text)
    return stddev, start


def clip_norm_key(conf):
    """the `clip_gradient_norm` key of the [trainer] section (a build addition like label_smoothing: absent from
    defaults/standardtrainer.cfg, off when absent or 0) -> c.  With c > 0 the update is clipped by the global L2 norm of
    its gradient instead of element by element: the mean over the update's A * world micro-batch gradients, unclipped,
    times min(1, c / its norm); an update whose norm is NaN or inf is skipped on the device."""
    text = str(conf.get('clip_gradient_norm', '0')).strip()
    try:
        c = float(text)
    except ValueError:
        raise ValueError('clip_gradient_norm must be a number, got %r' % text)
    if not (0.0 <= c < float('inf')):                           # (false for NaN)
        raise ValueError('clip_gradient_norm must be a finite norm >= 0 (0: off), got %r' % text)
    return c


def aggregate_key(conf, world):
    """the `numbatches_to_aggregate` key of the [trainer] section with `world` replicas -> A, the batches every replica
    takes per update.  0 (the default: defaults/standardtrainer.cfg) and `world` are the plain step (A = 1), A * world
    with A > 1 accumulates A clipped gradients per replica; everything else raises."""
    text = str(conf.get('numbatches_to_aggregate', '0')).strip()
    try:
        k = int(text)
    except ValueError:
        raise ValueError('numbatches_to_aggregate must be an integer, got %r (with %d replica%s)'
                         % (text, world, '' if world == 1 else 's'))
    if k < 0 or k % world:
        raise ValueError('numbatches_to_aggregate = %s with world = %d replica%s: the value must be 0 or a multiple of the '
                         'number of replicas (every replica then takes value / world batches per update); fewer '
                         'aggregated gradients than replicas would drop stale gradients as the reference\'s '
                         'SyncReplicasOptimizer does, which is not reproduced' % (text, world, '' if world == 1 else 's'))
    return max(k // world, 1)


def weight_noise_ranges(variables):
    """the range table of hip.weight_noise for variables laid out by VariableStore.flatten (each has .shape, .numel()
    and its .offset, a multiple of 4): sorted, disjoint [first_group, end_group) pairs in units of 4 elements over the
    variables with two or more dimensions — vectors (biases, layer-norm gains and offsets, attention_v) stay clean.
    Ranges that meet are joined.  A group holds one variable or padding: the last group of a matrix whose size is no
    multiple of 4 also holds padding and stays clean with it.  Host arithmetic only."""
    ranges = []
    for v in sorted(variables, key=lambda v: v.offset):
        if len(v.shape) < 2:
            continue
        if v.offset % 4:
            raise ValueError('variable %s starts at element %d of the flat buffer, not on a 16-byte group' % (v.name, v.offset))
        first, end = v.offset // 4, (v.offset + v.numel()) // 4
        if end <= first:
            continue
        if ranges and ranges[-1][1] == first:
            ranges[-1][1] = end
        else:
            ranges.append([first, end])
    return [tuple(r) for r in ranges]


class ValidationSaveHook(object):
    '''saves and restores the validated model (reference components/hooks.py:54-86: a
    tf.train.Saver over ALL global variables, i.e. weights, Adam slots, global step,
    learning-rate factor and the validation bookkeeping).  Kept in host memory when the
    trainer has no expdir.'''

    def __init__(self, filename, trainer):
        self.filename = filename
        self.trainer = trainer
        self._mem = None

    def save(self):
        st = self.trainer.state()
        if self.filename is None or self.trainer.task_index != 0:
            self._mem = st
        else:
            os.makedirs(os.path.dirname(self.filename), exist_ok=True)
            torch.save(st, self.filename)
            self._mem = st

    def restore(self):
        if self._mem is None and self.filename is not None and os.path.exists(self.filename):
            self._mem = torch.load(self.filename, weights_only=False)
        if self._mem is None:
            raise Exception('no validated model to restore')
        self.trainer.load_state(self._mem)


class DirectFeed(object):
    '''the batches of an update, read and uploaded on the loop's thread when the update asks for them'''

    def __init__(self, trainer):
        self.trainer = trainer

    def batches(self, first, n):
        tr = self.trainer
        return [tr.to_device(tr.data.batch(first + j * tr.world)) for j in range(n)]

    def close(self):
        pass


class AheadFeed(DirectFeed):
    '''the same batches staged by a BatchPrefetcher (Trainer.stage on its threads, `depth` ahead of the loop), uploaded
    with one copy and unpacked by one launch (Trainer.to_device_staged)'''

    def __init__(self, trainer, first, depth, pinned):
        from nabu_amd.processing.prefetch import BatchPrefetcher, PinnedRing
        DirectFeed.__init__(self, trainer)
        trainer._prefetcher = self.prefetcher = BatchPrefetcher(
            trainer.data, first, trainer.world, depth, int(trainer.conf.get('prefetch_workers', 2)), trainer.stage,
            PinnedRing(depth + 1) if pinned else None)

    def batches(self, first, n):
        if self.prefetcher.next_step != first:                  # a go-back restored an earlier global step
            self.prefetcher.reset(first)
        return [self.trainer.to_device_staged(self.prefetcher.get()) for _ in range(n)]

    def close(self):
        self.prefetcher.close()


class Trainer(object, metaclass=ABCMeta):
    '''General class outlining the training environment of a model.'''

    def __init__(self, conf, dataconf, modelconf, evaluatorconf, expdir, server, task_index):
        '''
        Args:
            conf: the trainer config as a ConfigParser ([trainer] section)
            dataconf: the data source: an object with ``batch(step)`` and
                ``num_batches()`` (e.g. processing.synthetic.SyntheticData), or a
                ConfigParser with a [synthetic] section describing one
            modelconf: the model configuration (ConfigParser: io/encoder/decoder)
            evaluatorconf: the evaluator configuration, None or evaluator = None
                disables validation
            expdir: directory where the model is written
            server: data-parallel process group (computing.dist.create_server())
                or None — replaces the tf.train.Server of the reference
            task_index: index of this worker (rank)
        '''
        self.conf = dict(conf.items('trainer'))
        apply_defaults(self.conf, defaults_path(__file__, self))
        self.dataconf = dataconf
        self.evaluatorconf = evaluatorconf
        self.expdir = expdir
        self.server = server
        self.world = server.world_size if server is not None else 1
        self.task_index = task_index
        if 'norm_constraint' in self.conf and self.conf['norm_constraint'] != 'None':
            raise Exception('norm_constraint (MaxNorm) is off by default in the reference '
                            '(standardtrainer.cfg:18) and not on the MI355X hot path')
        if int(self.conf['cut_sequence_length']):
            # reference trainer.py:364-384, 917-973: needs frame-synchronous targets (assert_equal over all
            # sequence lengths) and cannot build its graph on the pinned stack (tf.ceil over an int32
            # floor division, trainer.py:929) -- a non-zero key raises there too
            raise Exception('cut_sequence_length is not supported (it requires inputs and targets of equal '
                            'lengths and fails at graph construction in the reference, DESIGN.md section 8)')
        # label_smoothing (an extension key, absent from the defaults file, 0 when absent): validated here, and
        # together with the loss it cannot apply to (CTC), so that a bad configuration fails before the first step
        self.label_smoothing = loss_functions.label_smoothing_key(self.conf)
        if self.label_smoothing:
            loss_functions.factory(self.conf['loss'], self.label_smoothing)
        # ctc_weight (an extension key as well): the weight of the auxiliary CTC loss on the model's CTC head, validated
        # here with the loss it cannot apply to (CTC) and, below, with the model that must carry the head
        self.ctc_weight = loss_functions.ctc_weight_key(self.conf)
        if self.ctc_weight:
            loss_functions.factory(self.conf['loss'], self.label_smoothing, self.ctc_weight)
        # weight_noise / weight_noise_start_step (extension keys as well): validated here for the same reason
        self.weight_noise, self.weight_noise_start_step = weight_noise_keys(self.conf)
        self.flat_clean = self.noise_table = None
        # mwer_nbest / mwer_max_steps / mwer_ce_weight / mwer_start_step (extension keys as well, validated here too):
        # from global step mwer_start_step on, the step's loss is the expected number of label errors over the N-best
        # list of the model's own beam search (trainers/mwer.py); None without mwer_nbest
        self.mwer = mwer.mwer_keys(self.conf)
        self._mwer_stats = None            # device tensors of the latest MWER step (mwer_stats)
        if self.mwer is not None:
            if self.conf['loss'] == 'CTC':
                raise ValueError('mwer_nbest fine-tunes a model trained on a cross-entropy loss through its recurrent '
                                 'decoder; loss = CTC has no such decoder')
            if self.conf['loss'] == 'transducer':
                raise ValueError('mwer_nbest fine-tunes a model trained on a cross-entropy loss through its recurrent '
                                 'attention decoder; loss = transducer has no such decoder')
            if self.label_smoothing:
                raise ValueError('mwer_nbest does not combine with label_smoothing yet')
            if self.ctc_weight:
                raise ValueError('mwer_nbest does not combine with ctc_weight yet')
        # numbatches_to_aggregate: A batches per replica and update (1: the plain step), validated here as well
        self.accumulate = aggregate_key(self.conf, self.world)
        self.flat_acc = None               # the sum of an update's clipped micro-batch gradients (allocated when A > 1)
        self._micro = 0                    # micro-batches of the current update already in flat_acc
        # clip_gradient_norm (an extension key as well, validated here too): c > 0 clips the update's mean gradient by its
        # global norm and switches the element clip off.  The existing kernels then receive clip = +inf, with which
        # clip_value is the identity bit for bit: fminf(fmaxf(x, -inf), inf) == x, and NaN passes through as always.
        self.clip_norm = clip_norm_key(self.conf)
        self.clip = math.inf if self.clip_norm > 0 else CLIP
        self.clip_stats = self.clip_ws = None     # device words (norm, factor, skipped, 0) and the reduction's workspace
        self._skipped_reported = 0
        self.last_weight_noise = None      # the (seed, offset) of the latest noisy step
        self._noisy = False                # True from a step's noise launch until its optimiser has run
        self.model = Model(conf=modelconf, trainlabels=int(self.conf['trainlabels']), constraint=None)
        loss_functions.check_model(self.conf['loss'], self.model.decoder)
        if self.ctc_weight and not self.model.decoder.ctc_head:
            raise ValueError('ctc_weight = %g needs a model with a CTC head: set ctc_head = True in the [decoder] '
                             'section of the model' % self.ctc_weight)
        if self.mwer is not None:
            mwer.check_model(self.model)
        if bool(getattr(server, 'shared_devices', False)):
            # ranks that share a GPU (more ranks than devices on this node: first-contact runs, tests): the persistent
            # recurrent kernels need every CU of the device for their own workgroups, two processes' launches would each
            # hold a part of it and spin into the bounded time-out — decided HERE, where the process group is known, for
            # every layer this process builds (training and validation alike)
            from nabu_amd.neuralnetworks.components import layer as _layer
            _layer.LSTM_MODE[0] = hip.LSTM_STEPWISE
        self._graph = None
        self.schedule_log = None       # a list here records the bucketed exchange: (bucket key, 'hook' | 'final')

    # ------------------------------------------------------------------ graph
    def _create_graph(self):
        '''set up everything one step needs (the analogue of building the TF graph,
        reference trainer.py:73-283)'''
        if self._graph is not None:
            return self._graph
        outputs = {}
        self.global_step = 0
        self.adam_step = 0
        self.learning_rate_fact = 1.0
        self.data = self._data()
        outputs['num_steps'] = self.data.num_batches() * int(self.conf['num_epochs'])
        if self.accumulate > 1:            # updates, A batches each: the data seen stays that of num_epochs
            outputs['num_steps'] = max(1, outputs['num_steps'] // self.accumulate)
        self.loss_fn = loss_functions.factory(self.conf['loss'], self.label_smoothing, self.ctc_weight)
        self.flat = self.flat_grad = self.adam_m = self.adam_v = None
        self.buckets = None
        # validation part (reference trainer.py:189-265): bookkeeping 'variables' of the
        # validate/ scope with the reference's initial values
        self.evaluator = None
        if (self.evaluatorconf is not None and self.evaluatorconf.has_section('evaluator')
                and self.evaluatorconf.get('evaluator', 'evaluator') != 'None'):
            self.evaluator = self._validate()
        self.validated_step = -int(self.conf['valid_frequency'])
        self.best_validation = 1.79e+308
        self.num_tries = 0
        self.validation_hook = ValidationSaveHook(
            None if self.expdir is None else os.path.join(self.expdir, 'logdir', 'validated.ckpt'), self)
        self._graph = outputs
        return outputs

    def _validate(self):
        '''create the evaluator (reference trainer.py:459-477)'''
        from nabu_amd.neuralnetworks.evaluators import evaluator_factory
        evaltype = self.evaluatorconf.get('evaluator', 'evaluator')
        # a synthetic batch source derives its own validation set; on-disk data are described by
        # the database conf (dev sections named in the evaluator conf)
        dataconf = self.data if hasattr(self.data, 'validation') else self.dataconf
        return evaluator_factory.factory(evaltype)(conf=self.evaluatorconf, dataconf=dataconf, model=self.model)

    def validation_loss(self):
        '''run the evaluator over the validation set (reference trainer.py:660-680)'''
        loss, update_loss, valbatches = self.evaluator.evaluate()
        for i in range(valbatches):
            update_loss(i)
        return loss[0]

    def _data(self):
        '''the batch source (reference trainer.py:285-423 builds the queue-runner
        pipeline here)'''
        d = self.dataconf
        if hasattr(d, 'batch') and hasattr(d, 'num_batches'):
            return d
        if hasattr(d, 'has_section') and d.has_section('synthetic'):
            from nabu_amd.processing.synthetic import SyntheticData
            def value(v):
                if v in ('True', 'False'):
                    return v == 'True'
                try:
                    return int(v)
                except ValueError:
                    return v                   # names (input_name, target_name = alignments)
            kw = {k: value(v) for k, v in d.items('synthetic')}
            kw.setdefault('batch_size', int(self.conf['batch_size']))
            return SyntheticData(**kw)
        # the reference's on-disk data (reference trainer.py:289-340): the trainer conf links the model's
        # input names and the target names to sections of database.conf
        from nabu_amd.processing import input_pipeline
        input_names = [n for n in self.model.conf.get('io', 'inputs').split(' ') if n]
        target_names = [n for n in self.conf['targets'].split(' ') if n]
        return input_pipeline.from_sections(
            d, input_names, [self.conf[i].split(' ') for i in input_names],
            target_names, [self.conf[o].split(' ') for o in target_names],
            batch_size=int(self.conf['batch_size']), numbuckets=int(self.conf['numbuckets']),
            variable_batch_size=self.conf['variable_batch_size'] == 'True', shuffle=True, seed=0)

    def learning_rate(self):
        '''exponential decay (non-staircase) times the validation factor
        (reference trainer.py:153-166)'''
        num_steps = self._graph['num_steps']
        return (float(self.conf['initial_learning_rate'])
                * float(self.conf['learning_rate_decay']) ** (float(self.global_step) / num_steps)
                * self.learning_rate_fact)

    def to_device(self, batch, device=None):
        '''numpy batch (A0 contract) -> device tensors / SeqLen objects'''
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        out = {}
        for key in ('inputs', 'targets'):
            out[key] = {}
            for n, a in batch[key].items():
                if isinstance(a, torch.Tensor):
                    out[key][n] = a.to(device)
                else:
                    dt = torch.float32 if key == 'inputs' else torch.int32
                    out[key][n] = torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(device)
        for key in ('input_seq_length', 'target_seq_length'):
            out[key] = {n: SeqLen.wrap(a, device) for n, a in batch[key].items()}
        return out

    # ------------------------------------------------------------------- step
    def step(self, batch):
        '''one training update on a device batch; returns the loss as a 1-element
        device tensor (no host synchronisation)'''
        self._create_graph()
        if self.accumulate > 1:
            raise ValueError('step takes one batch per update; this trainer takes %d (numbatches_to_aggregate = %s with '
                             '%d replicas): call step_accumulated()'
                             % (self.accumulate, self.conf['numbatches_to_aggregate'], self.world))
        return self._run_update([batch])

    def step_accumulated(self, batches):
        '''one training update on numbatches_to_aggregate / replicas = A device batches (A > 1), taken one after another:
        each micro-batch runs the forward pass, the loss and the backward pass of step(), its gradient is clipped and
        added to flat_acc in the order of the list, the last one ends in the exchange and ONE Adam step on the mean.
        Weight noise is drawn once, before the first micro-batch; the model's own draws come per micro-batch.  Returns
        the mean of the A losses as a 1-element device tensor (no host synchronisation).'''
        self._create_graph()
        if self.accumulate < 2:
            raise ValueError('step_accumulated needs numbatches_to_aggregate = A * replicas with A > 1; this trainer '
                             'takes one batch per update: call step()')
        if len(batches) != self.accumulate:
            raise ValueError('step_accumulated takes %d batches per update (numbatches_to_aggregate = %s with %d '
                             'replicas), got %d' % (self.accumulate, self.conf['numbatches_to_aggregate'], self.world,
                                                    len(batches)))
        if self._micro:
            raise Exception('an update is under way (%d micro-batches accumulated)' % self._micro)
        return self._run_update(batches)

    def _forward_loss(self, batch):
        '''the forward pass and the loss of one device batch -> (tape, loss).  With mwer_nbest, from global step
        mwer_start_step on, the pass is trainers/mwer.py's; before it, and without the key, the calls below are the ones
        they always were'''
        if self.mwer is not None and self.global_step >= self.mwer[3]:
            with Tape() as tape:
                loss, self._mwer_stats = mwer.forward_loss(self.model, batch, *self.mwer[:3])
                extra = self.aditional_loss()
                if extra is not None:
                    loss = hip.axpy_(loss, extra)
            return tape, loss
        with Tape() as tape:
            logits, logit_seq_length = self.model(
                inputs=batch['inputs'], input_seq_length=batch['input_seq_length'],
                targets=batch['targets'], target_seq_length=batch['target_seq_length'],
                is_training=True)
            loss = self.loss_fn(batch['targets'], logits, logit_seq_length, batch['target_seq_length'])
            extra = self.aditional_loss()
            if extra is not None:
                loss = hip.axpy_(loss, extra)
        return tape, loss

    def _run_update(self, batches):
        '''the body of step ([batch]) and step_accumulated (A batches): every batch but the last accumulates, the last
        one updates (_backward_and_update); returns the loss, of several batches their mean'''
        if self.weight_noise > 0 and self.global_step >= self.weight_noise_start_step:
            self._add_weight_noise(batches[0])
        total = None
        try:
            for batch in batches:
                tape, loss = self._forward_loss(batch)
                if self.flat is None:
                    self._init_optimizer()
                self._backward_and_update(tape, loss)
                if len(batches) > 1:
                    total = loss if total is None else hip.axpy_(total, loss)
            return loss if total is None else hip.sum_(total, 1.0 / len(batches))
        finally:
            self._micro = 0            # (an exception: the partial sum is dropped, micro-batch 0 overwrites flat_acc)
            if self._noisy:            # raised between the noise launch and the optimiser: back to the clean parameters
                self._noisy = False
                self.flat.copy_(self.flat_clean)

    def _add_weight_noise(self, batch):
        '''a noisy step (the keys weight_noise / weight_noise_start_step): ONE offset of the global stream, taken before
        the model's own draws, then ONE launch that saves the flat parameters to flat_clean and adds
        weight_noise * N(0, 1) to every matrix in place.  The forward and backward passes of this step run at the noisy
        values; _update computes the new parameters from flat_clean, so between steps flat is always clean.'''
        from nabu_amd.neuralnetworks.components import ops as nops
        seed, offset = nops.global_rng().next()
        if self.flat is None:
            if not self.model.store.order:
                # the noise needs the variables before the training forward pass that would create them: created as
                # _ensure_variables does (a forward pass that is not training, here on the step's own batch), and
                # the stream stays where it was
                kept = nops.global_rng().offset
                with torch.no_grad():
                    self.model(batch['inputs'], batch['input_seq_length'], batch['targets'],
                               batch['target_seq_length'], False)
                nops.global_rng().offset = kept
            self._init_optimizer()
        hip.weight_noise(self.flat, self.flat_clean, self.noise_table, self.weight_noise, seed, offset)
        self._noisy = True
        self.last_weight_noise = (seed, offset)

    def _backward_and_update(self, tape, loss):
        last = self._micro == self.accumulate - 1          # (always, without accumulation)
        hooked = self.buckets is not None and last         # buckets travel under the LAST micro-batch's backward pass
        if hooked:
            self._begin_bucketed(tape)
        try:
            tape.backward(loss)
        finally:
            if hooked:
                self._end_backward()
                failed = hip.take_phase_hook_error()      # raised inside the C -> Python hook of nabu_blstm_bwd
                if failed is not None:
                    self._join_comm()                     # no collective outlives the step
                    raise failed
        if last:
            self._update()
        else:
            self._accumulate(self._micro)

    def _accumulate(self, j):
        '''micro-batch j < A - 1 of an update: flat_acc (+)= clip(flat_grad), one launch; j = 0 writes the accumulator
        without reading it.  The last micro-batch goes to _update.'''
        if self.accumulate < 2 or j != self._micro or j >= self.accumulate - 1:
            raise Exception('micro-batch %d cannot be accumulated: %d of %d are in, the last one belongs to the update'
                            % (j, self._micro, self.accumulate))
        if self.flat_acc is None:
            self.flat_acc = torch.empty_like(self.flat_grad)
        hip.clip_accumulate(self.flat_acc, self.flat_acc if j else None, self.flat_grad, self.clip)
        self._micro = j + 1

    def _init_optimizer(self):
        store = self.model.store
        self.flat, self.flat_grad = store.flatten()
        self.adam_m = torch.zeros_like(self.flat)
        self.adam_v = torch.zeros_like(self.flat)
        if self.world > 1:
            self.server.broadcast_(self.flat, 0)       # identical replicas
        self.buckets = None
        if self.world > 1 and self.conf.get('allreduce_buckets', 'False') == 'True':
            self.buckets = self._make_buckets()
        if self.weight_noise > 0:          # (a configuration without the key allocates neither)
            self.flat_clean = torch.empty_like(self.flat)
            self.noise_table = hip.WeightNoiseTable(weight_noise_ranges(store.trainable_variables()), self.flat.device)
            if self.noise_table.n > hip.WEIGHT_NOISE_MAX_RANGES:
                raise ValueError('weight_noise: the matrices form %d separate ranges of the flat parameter buffer, the '
                                 'kernel takes %d' % (self.noise_table.n, hip.WEIGHT_NOISE_MAX_RANGES))
        if self.clip_norm > 0:             # (nor these two)
            self.clip_stats, self.clip_ws = hip.grad_norm_buffers(self.flat_grad.numel(), self.flat_grad.device)

    # ----------------------------------------------------- bucketed gradient exchange
    @staticmethod
    def bucket_key(name):
        '''variables of one encoder layer share a bucket (<encoder>/<input>/layer<l>), everything
        else (the decoder) forms one more'''
        parts = name.split('/')
        return '/'.join(parts[:3]) if len(parts) > 3 and parts[2].startswith('layer') else 'decoder'

    def _make_buckets(self):
        '''contiguous ranges of the flat gradient buffer, in variable-creation order'''
        buckets = []
        for v in self.model.store.trainable_variables():
            key = self.bucket_key(v.name)
            end = v.offset + (v.numel() + 3) // 4 * 4
            if buckets and buckets[-1]['key'] == key and buckets[-1]['end'] == v.offset:
                buckets[-1]['end'] = end
                buckets[-1]['vars'].append(v)
            else:
                buckets.append(dict(key=key, start=v.offset, end=end, vars=[v]))
        assert buckets[0]['start'] == 0 and buckets[-1]['end'] == self.flat_grad.numel()
        return buckets

    def _begin_bucketed(self, tape):
        self._ready = set()            # ids of variables whose gradient is final
        self._sent = set()             # bucket indices already on the wire
        self._works = []
        self._declared = {id(v) for op in tape.ops for v in op.params}
        tape.on_param_ready = lambda v: self._ready.add(id(v))
        # weight-gradient products deferred behind the last recurrence (layer.py, Tape.defer): a layer's bucket goes on
        # the wire right after its products and travels under the next layer's
        tape.after_deferred = self._launch_ready_buckets
        hip.set_phase_hook(self._launch_ready_buckets)
        hip.BEFORE_RECURRENT[0] = self._join_comm

    def _end_backward(self):
        hip.set_phase_hook(None)
        hip.BEFORE_RECURRENT[0] = None
        if sys.exc_info()[0] is not None:                 # the backward pass raised: drain what is in flight
            try:
                self._join_comm()
            except Exception:                             # the original error is the one to report
                pass

    def _launch_ready_buckets(self, everything=False):
        '''clip (per replica, before the aggregation: reference trainer.py:556-569) and start the
        all-reduce of every bucket whose gradients are final.  Called between a recurrent kernel and
        the dense products that follow it (nabu_blstm_set_phase_hook) and once after the backward pass.'''
        for i, b in enumerate(self.buckets):
            if i in self._sent:
                continue
            if not everything and not all(id(v) in self._ready and id(v) in self._declared for v in b['vars']):
                continue
            self._works.append(self.server.all_reduce_sum_async(self._clip_local(b['start'], b['end'])))
            self._sent.add(i)
            if self.schedule_log is not None:       # (bench.py / tests: which bucket went on the wire at which call)
                self.schedule_log.append((b['key'], 'final' if everything else 'hook'))

    def _clip_local(self, start, end):
        '''what this replica sends of flat_grad[start:end], left there: the clipped gradient (clip per replica, before the
        aggregation), with A > 1 the local sum of A clipped gradients; returns the view.  With clip_gradient_norm the
        element clip is off (self.clip is +inf): the sum is that of the plain gradients, and a single one is sent as it
        is, without a launch'''
        view = self.flat_grad[start:end]
        if self.accumulate > 1:
            hip.clip_accumulate(view, self.flat_acc[start:end], view, self.clip)
        elif not self.clip_norm > 0:
            hip.clip_(view, CLIP)
        return view

    def _join_comm(self):
        '''the launch stream waits for every exchange in flight (before a recurrent launch and
        before the optimiser)'''
        works, self._works = self._works, []
        for w in works:
            if w is not None:
                w.wait()

    def _update(self):
        '''clip + Adam (reference trainer.py:512-580) behind the last (without accumulation: the only) micro-batch of an
        update, with the gradient exchange of the data-parallel mode in between.  flat_grad holds that micro-batch's
        gradient as the backward pass left it, flat_acc the A - 1 clipped ones before it.  One replica: ONE launch clips,
        adds and applies Adam.  Several: every replica completes its clipped local sum in flat_grad (_clip_local; per
        bucket under the backward pass and here for the rest), the sums are exchanged ONCE, and Adam runs on
        1 / (A * world) of the total: the mean of A * world clipped gradients, what A * world replicas compute.
        With clip_gradient_norm = c the same path runs with the element clip off (self.clip = +inf; a single replica's
        lone gradient is not touched before the exchange) and one grad_norm call behind the exchange: Adam then runs on
        the plain mean times min(1, c / its L2 norm), or not at all when that norm is not finite (_adam).'''
        A = self.accumulate
        if self._micro != A - 1:
            raise Exception('the update needs %d accumulated micro-batches, %d are in' % (A - 1, self._micro))
        lr = self.learning_rate()
        self.adam_step += 1
        lr_t = lr * math.sqrt(1.0 - ADAM_B2 ** self.adam_step) / (1.0 - ADAM_B1 ** self.adam_step)
        acc = self.flat_acc if A > 1 else None
        if self.world > 1:
            if self.buckets is None:
                self._clip_local(0, self.flat_grad.numel())      # a local launch: outside the timed exchange
            ev = self._allreduce_events()                        # exposed part of the exchange only
            if self.buckets is None:
                self.server.all_reduce_sum_(self.flat_grad)      # sum over xGMI
            else:
                self._launch_ready_buckets(everything=True)
                self._join_comm()
            if ev is not None:
                ev[1].record()
            acc = None                                           # (in the exchanged sum)
        if self.clip_norm > 0:
            # the norm of the mean gradient and the factor the update applies, left on the device: behind the exchange,
            # so every replica reduces the same sum in the same order and gets the same bits
            hip.grad_norm(self.flat_grad, acc, 1.0 / (A * self.world), self.clip_norm, self.clip_stats, self.clip_ws)
        self._adam(lr_t, 1.0 / (A * self.world), acc)
        self._micro = 0
        self.last_lr = lr

    def _adam(self, lr_t, scale, acc):
        '''the fused clip + Adam launch on scale * flat_grad, with `acc` on scale * (acc + clip(flat_grad)); after a noisy
        step (_add_weight_noise) the parameter is read from the clean copy, so the noise leaves with the update and
        nothing has to be subtracted again.  With clip_gradient_norm: ONE entry point for the same src / acc choice,
        no clamp, and the scale is the factor grad_norm left on the device (scale * min(1, c / norm)); a factor of NaN
        (a norm that is not finite) skips the update there: m, v and the clean parameters stay as they are, nothing is
        read back, and adam_step has advanced all the same, so the bias correction of later updates is that of one
        more step'''
        src = self.flat_clean if self._noisy else None
        rest = (self.adam_m, self.adam_v, lr_t, ADAM_B1, ADAM_B2, ADAM_EPS, CLIP, scale)
        if self.clip_norm > 0:
            hip.adam_scaled_step(self.flat, src, acc, self.flat_grad, self.adam_m, self.adam_v, lr_t, ADAM_B1, ADAM_B2,
                                 ADAM_EPS, self.clip_stats)
        elif acc is not None:
            hip.adam_clip_step_acc(self.flat, src, acc, self.flat_grad, *rest)
        elif src is not None:
            hip.adam_clip_step_from(self.flat, src, self.flat_grad, *rest)
        else:
            hip.adam_clip_step(self.flat, self.flat_grad, *rest)
        self._noisy = False

    def grad_stats(self):
        '''(norm, factor, skipped) of the latest update with clip_gradient_norm: the L2 norm of its mean gradient, the
        factor the gradient sum was multiplied by (NaN: the update was skipped) and the number of updates skipped so far.
        Copies four words to the host, so it synchronises; train() does not call it per step.'''
        if self.clip_stats is None:
            raise Exception('grad_stats needs clip_gradient_norm > 0 and a first update')
        return hip.read_grad_stats(self.clip_stats)

    def mwer_stats(self):
        '''(mean expected errors, mean reference nll, share of valid hypotheses) of the latest MWER step.  Copies three
        words to the host, so it synchronises; train() does not call it per step.'''
        if self._mwer_stats is None:
            raise Exception('mwer_stats needs mwer_nbest > 0 and a first MWER step (global step >= mwer_start_step)')
        return mwer.read_stats(self._mwer_stats)

    def _report_skipped(self):
        '''called where train() has synchronised anyway (a validation point, the end): says so when updates were skipped
        since the last report'''
        if self.clip_stats is None:
            return
        skipped = hip.read_grad_stats(self.clip_stats)[2]
        if skipped != self._skipped_reported:
            print('WORKER %d: %d updates skipped (non-finite gradient norm)' % (self.task_index, skipped))
            self._skipped_reported = skipped

    def _allreduce_events(self):
        '''bench.py sets ``time_allreduce``: a pair of events on the launch stream around the
        exchange (the collective's own stream is joined to it by torch.distributed)'''
        if not getattr(self, 'time_allreduce', False) or not torch.cuda.is_available():
            return None
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        if not hasattr(self, 'allreduce_ms'):
            self.allreduce_ms = []
        self.allreduce_ms.append(ev)
        return ev

    # ------------------------------------------------------- state (checkpoints)
    def state(self):
        '''everything tf.train.Saver() of the reference's session would write: model
        variables, Adam slots, global step, learning-rate factor, validation bookkeeping'''
        if self._micro:
            raise Exception('state() in the middle of an update (%d of %d micro-batches accumulated): checkpoints fall '
                            'on update boundaries' % (self._micro, self.accumulate))
        if self.flat is None:
            self._init_optimizer()
        from nabu_amd.neuralnetworks.components import ops as nops
        return dict(names=list(self.model.store.order), flat=self.flat.detach().cpu().clone(),
                    adam_m=self.adam_m.cpu().clone(), adam_v=self.adam_v.cpu().clone(),
                    global_step=self.global_step, adam_step=self.adam_step,
                    learning_rate_fact=self.learning_rate_fact, validated_step=self.validated_step,
                    best_validation=self.best_validation, rng_offset=nops.global_rng().offset)

    def load_state(self, st):
        if self.flat is None:
            self._init_optimizer()
        if list(st['names']) != list(self.model.store.order) or st['flat'].numel() != self.flat.numel():
            raise Exception('checkpoint does not match the model (variable names / sizes differ)')
        from nabu_amd.neuralnetworks.components import ops as nops
        self.flat.copy_(st['flat'])
        self.adam_m.copy_(st['adam_m'])
        self.adam_v.copy_(st['adam_v'])
        self.global_step, self.adam_step = int(st['global_step']), int(st['adam_step'])
        self.learning_rate_fact = float(st['learning_rate_fact'])
        self.validated_step = int(st['validated_step'])
        self.best_validation = float(st['best_validation'])
        nops.global_rng().offset = int(st['rng_offset'])

    def _ensure_variables(self):
        '''variables are created by the first call of the model (the reference creates them
        when it builds the graph): run one forward pass if that has not happened yet'''
        if self.flat is None and not self.model.store.order:
            b = self.to_device(self.data.batch(0))
            with torch.no_grad():
                self.model(b['inputs'], b['input_seq_length'], b['targets'], b['target_seq_length'], False)

    def _validation_point(self):
        '''the validation branch of the training loop (reference trainer.py:646-737).
        Every replica evaluates the same validation set on identical weights, so all of them
        take the same decision (the reference lets the chief decide and the others wait).
        Returns True when training must terminate.'''
        print('WORKER %d: validating model' % self.task_index)
        prev_val_loss = self.best_validation
        validation_loss = self.validation_loss()
        print('WORKER %d: validation loss: %f' % (self.task_index, validation_loss))
        self.validation_history.append((self.global_step, validation_loss))
        if validation_loss >= prev_val_loss:
            print('WORKER %d: validation loss is worse' % self.task_index)
            if self.conf['num_tries'] != 'None':
                if self.num_tries == int(self.conf['num_tries']):
                    self.validation_hook.restore()
                    print('WORKER %d: terminating training' % self.task_index)
                    return True
            self.num_tries += 1
            if self.conf['go_back'] == 'True':
                print('WORKER %d: loading previous model' % self.task_index)
                self.validation_hook.restore()
            else:
                self.validated_step = self.global_step
            if self.conf['valid_adapt'] == 'True':
                print('WORKER %d: halving learning rate' % self.task_index)
                self.learning_rate_fact /= 2
                self.validation_hook.save()
        else:
            if self.conf['reset_tries'] == 'True':
                self.num_tries = 0
            self.validated_step = self.global_step
            self.best_validation = validation_loss
            self.validation_hook.save()
        return False

    # ------------------------------------------------------------------ train
    def train(self, testing=False):
        '''train the model (reference trainer.py:582-792)

        args:
            testing: if true only the "graph" is created, for debugging purposes
        returns: the list of (global_step, loss, learning_rate) that was printed'''
        outputs = self._create_graph()
        if testing:
            return []
        is_chief = self.task_index == 0
        history = []
        self.validation_history = []
        num_steps = outputs['num_steps']
        # MonitoredTrainingSession(checkpoint_dir=expdir/logdir) restores the latest checkpoint
        # when one exists (reference trainer.py:625-633) and saves one every 600 s
        ckpt = None if self.expdir is None else os.path.join(self.expdir, 'logdir', 'model.ckpt')
        if ckpt is not None and os.path.exists(ckpt):
            self._ensure_variables()
            self.load_state(torch.load(ckpt, weights_only=False))
            print('WORKER %d: resumed from %s at step %d' % (self.task_index, ckpt, self.global_step))
        on_gpu = torch.cuda.is_available()
        mem_total = torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory if on_gpu else 0

        def shard():
            # each replica reads its own shard of the epoch (replaces the shared filename queue on ps:0,
            # trainer.py:342-351).  Update s, micro-batch j, rank r: batch (s * A + j) * world + r, what A * world
            # replicas read; this is the first of update global_step, the others follow `world` apart
            return self.global_step * self.accumulate * self.world + self.task_index

        def reduce(loss):
            return self.server.all_reduce_sum_(loss.clone()) if self.world > 1 else loss

        def report(step, loss_sum, lr, start):
            loss_value = loss_sum / self.world
            mem_used = torch.cuda.max_memory_allocated() if on_gpu else 0
            print(('WORKER %d: step %d/%d loss: %f, learning rate: %f \n\t time elapsed: %f sec'
                   '\n\t peak memory usage: %d/%d MB')
                  % (self.task_index, step, num_steps, loss_value, lr, time.time() - start, mem_used / 1e6,
                     mem_total / 1e6))
            history.append((step, loss_value, lr))

        # the reference's loop reads a batch when the step asks for it and the loss at once; the extension key
        # prefetch_batches = N >= 1 has batches staged N ahead and reads a step's words one step late (DESIGN.md
        # section 8): history, validation decisions and checkpoints are the same, an infeasible CTC batch or a
        # persistent kernel's time-out raises one iteration late, naming its step
        depth = int(self.conf.get('prefetch_batches', 0))
        feed = AheadFeed(self, shard(), depth, on_gpu) if depth > 0 else DirectFeed(self)
        reader = readback.ReadLate(reduce, report, on_gpu) if depth > 0 else readback.ReadNow(reduce, report)
        last_ckpt = time.time()
        try:
            while self.global_step < num_steps:
                if (self.evaluator is not None
                        and self.global_step - self.validated_step >= int(self.conf['valid_frequency'])):
                    reader.drain()
                    self._report_skipped()
                    self._ensure_variables()
                    if self._validation_point():
                        break
                start = time.time()
                batches = feed.batches(shard(), self.accumulate)
                loss = self.step(batches[0]) if self.accumulate == 1 else self.step_accumulated(batches)
                reader.push(self.global_step, loss, self.last_lr, start)
                self.global_step += 1
                reader.drain(reader.lag)                        # with a lag: read step s now that step s + 1 is enqueued
                every = getattr(self, 'checkpoint_steps', None)
                if is_chief and ckpt is not None and (
                        time.time() - last_ckpt > CHECKPOINT_SECS or (every and self.global_step % every == 0)):
                    reader.drain()
                    self.save_checkpoint(ckpt)
                    last_ckpt = time.time()
            reader.drain()
            self._report_skipped()
        finally:
            feed.close()
        if is_chief and self.expdir is not None:
            self.save_checkpoint(ckpt)
            self.save()
        return history

    # ------------------------------------------------- staged batches (prefetch_batches >= 1)
    def stage(self, batch, slot=None):
        '''numpy batch -> packed batch (processing/prefetch.py), written into the pinned `slot` when one is given.
        Runs on a prefetcher thread: no device call in here.'''
        from nabu_amd.processing import prefetch
        return prefetch.stage(batch, slot)

    def to_device_staged(self, staged, device=None):
        '''packed batch -> what to_device returns for the same batch: ONE asynchronous upload on the launch stream
        and ONE launch (nabu_batch_unpack) that writes every padded tensor and length vector'''
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        n = staged.nbytes
        src = staged.slot.tensor if staged.slot is not None else torch.from_numpy(staged.array)
        packed = hip.Workspace.get(n, device, 'batch')
        packed[:n].copy_(src[:n], non_blocking=True)
        if staged.slot is not None:                       # the slot is free again once this copy has read it
            uploaded = torch.cuda.Event()
            uploaded.record()
            staged.slot.uploaded(uploaded)
        out = dict(inputs={}, targets={}, input_seq_length={}, target_seq_length={})
        segs = []
        for s in staged.segments:
            data = torch.empty(s.shape, dtype=torch.float32 if s.key == 'inputs' else torch.int32, device=device)
            lens = torch.empty(s.rows, dtype=torch.int32, device=device)
            segs.append(s.describe() + (data, lens))
            out[s.key][s.name] = data
            out['input_seq_length' if s.key == 'inputs' else 'target_seq_length'][s.name] = SeqLen(
                np.clip(s.lengths, 0, s.max_len), dev_tensor=lens)
        for i in range(0, len(segs), 8):                  # NABU_BATCH_MAX_SEGS per launch
            hip.batch_unpack(segs[i:i + 8], packed, n)
        return out

    def save_checkpoint(self, path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save(self.state(), path + '.tmp')
        os.replace(path + '.tmp', path)

    def save(self):
        '''final model: variables by TF-style name (SaveAtEnd, hooks.py:30-52) and
        the pickled model configuration (trainer.py:789-792)'''
        mdir = os.path.join(self.expdir, 'model')
        os.makedirs(mdir, exist_ok=True)
        np.savez(os.path.join(mdir, 'network.ckpt.npz'), **self.model.store.state_dict())
        with open(os.path.join(mdir, 'model.pkl'), 'wb') as fid:
            pickle.dump({s: dict(self.model.conf.items(s)) for s in self.model.conf.sections()}, fid)

    @abstractmethod
    def aditional_loss(self):
        '''an additional loss term or None'''

    @abstractmethod
    def chief_only_hooks(self, outputs):
        '''hooks for the chief worker only'''

    @abstractmethod
    def hooks(self, outputs):
        '''hooks for every worker'''
