"""
The scaffold the four semi-supervised trainers share (cutmix-semisup-seg_amd/trainer_common.py), on the CPU:

  * the complete option tables against tests/golden/trainer_cli_full.json, written by tests/golden/make_trainer_cli_golden.py
    from the commit before the tables were shared (order, names, opts, types, defaults, flags, choices -- this build's own
    options and their positions included, which the reference goldens do not pin);
  * the epoch bookkeeping (accumulate / epoch_means / network_dead / epoch_line) fed with hand-written step results. The expected
    figures restate the arithmetic of the trainers' former loops line by line in plain Python floats; every input is a binary
    fraction, so the float64 sums are exact and the comparisons are equalities.

run_epochs itself is not run on real networks here (its evaluator histograms on the GPU); one test drives it with placeholder
modules and a stand-in evaluator for the order of its checks and its log lines.
"""
import inspect
import math

import click
import numpy as np
import pytest
import torch

from conftest import load_golden_json
from cutmix_semisup_seg_amd import trainer_common as tc

# (trainer module, does a NaN consistency loss end the job, is step.nan_detected() polled every iteration): as each trainer had
# it before the loop was shared -- inherited, not chosen
NAN_POLICIES = [('train_seg_semisup_mask_mt', False, True), ('train_seg_semisup_vat_mt', True, False),
                ('train_seg_semisup_ict', True, False), ('train_seg_semisup_aug_mt', True, False)]


@pytest.mark.parametrize('name', [p[0] for p in NAN_POLICIES])
def test_full_option_table_matches_the_snapshot(name):
    trainer = __import__(name)
    got = []
    for prm in trainer.experiment.params:
        choices = list(prm.type.choices) if isinstance(prm.type, click.Choice) else None
        got.append(dict(name=prm.name, opts=list(prm.opts), type=type(prm.type).__name__,
                        default=prm.default if isinstance(prm.default, (bool, int, float, str)) else None,
                        is_flag=bool(getattr(prm, 'is_flag', False)), choices=choices))
    want = load_golden_json('trainer_cli_full')[name]
    assert [o['name'] for o in got] == [o['name'] for o in want]
    for g, w in zip(got, want):
        assert g == w, g['name']
        assert type(g['default']) is type(w['default']), g['name']         # True is not 1, 1.0 is not 1
    assert trainer.experiment.name == 'experiment'


def former_epoch(results, n_unsup_each, ramp_val, conf_thresh, rampup):
    """The bookkeeping of the trainers' loops as it stood in each of the four files, on Python floats."""
    sup_sum = cons_sum = conf_sum = 0.0
    n_sup_batches = n_unsup_batches = 0
    for res, n_unsup in zip(results, n_unsup_each):
        sup_sum += float(res['sup_loss'])
        n_sup_batches += 1
        if res['consistency_loss'] is not None:
            cons_sum += float(res['consistency_loss'])
            if conf_thresh > 0.0:
                conf_sum += float(res['conf_rate'])
            elif rampup > 0:
                conf_sum += ramp_val
            n_unsup_batches += n_unsup
    sup_loss_acc = sup_sum / max(n_sup_batches, 1)
    consistency_loss_acc = cons_sum / max(n_sup_batches, 1) if n_unsup_batches > 0 else 0.0
    conf_rate_acc = conf_sum / max(n_sup_batches, 1) if n_unsup_batches > 0 else 0.0
    return (sup_loss_acc, consistency_loss_acc, conf_rate_acc), n_sup_batches, n_unsup_batches


def shared_epoch(results, n_unsup_each, ramp_val, conf_thresh, rampup):
    acc = torch.zeros(3, dtype=torch.float64, device='cpu')
    n_sup_batches = n_unsup_batches = 0
    for res, n_unsup in zip(results, n_unsup_each):
        n_sup_batches += 1
        n_unsup_batches += tc.accumulate(acc, res, n_unsup, ramp_val, conf_thresh, rampup)
    return tuple(float(v) for v in tc.epoch_means(acc, n_sup_batches, n_unsup_batches)), n_sup_batches, n_unsup_batches


def _res(sup, cons, conf):
    """A step result as the steps return it: 0-d float32 tensors, None where there was no unsupervised batch."""
    t = lambda v: None if v is None else torch.tensor(v, dtype=torch.float32)
    return dict(sup_loss=t(sup), consistency_loss=t(cons), conf_rate=t(conf))


WITH_UNSUP = [_res(1.5, 0.25, 0.5), _res(0.75, 0.125, 0.25), _res(2.0, 0.5, 1.0), _res(0.25, 0.0625, 0.0)]


def test_a_confidence_threshold_reports_the_confidence_rate():
    got = shared_epoch(WITH_UNSUP, [1] * 4, 0.375, 0.97, 5)
    assert got == former_epoch(WITH_UNSUP, [1] * 4, 0.375, 0.97, 5)
    assert got == ((4.5 / 4, 0.9375 / 4, 1.75 / 4), 4, 4)                   # conf_rate summed; the ramp value is not


def test_without_a_threshold_the_rate_column_carries_the_ramp_value():
    got = shared_epoch(WITH_UNSUP, [1] * 4, 0.375, 0.0, 5)
    assert got == former_epoch(WITH_UNSUP, [1] * 4, 0.375, 0.0, 5)
    assert got[0][2] == 0.375                                               # 4 x ramp / 4 iterations: the reference's quirk
    # no threshold and no ramp-up: nothing is added
    got = shared_epoch(WITH_UNSUP, [1] * 4, 1.0, 0.0, -1)
    assert got == former_epoch(WITH_UNSUP, [1] * 4, 1.0, 0.0, -1) and got[0][2] == 0.0


def test_no_unsupervised_batches_print_zero_for_both_consistency_figures():
    sup_only = [_res(1.5, None, None), _res(0.5, None, None)]
    got = shared_epoch(sup_only, [0, 0], 0.375, 0.97, 5)
    assert got == former_epoch(sup_only, [0, 0], 0.375, 0.97, 5)
    assert got == ((1.0, 0.0, 0.0), 2, 0)
    line = tc.epoch_line(0, 1.0, *got[0], 0.5)
    assert 'consistency loss=0.000000, conf rate=0.000%' in line


def test_a_missing_consistency_loss_leaves_the_unsupervised_count_alone():
    """The step returns consistency_loss None; the batches handed to it are then not counted."""
    mixed = [_res(1.0, None, None), _res(1.0, 0.5, 0.25), _res(1.0, None, None)]
    acc = torch.zeros(3, dtype=torch.float64)
    assert tc.accumulate(acc, mixed[0], 2, 1.0, 0.97, -1) == 0
    assert acc.tolist() == [1.0, 0.0, 0.0]
    assert tc.accumulate(acc, mixed[1], 2, 1.0, 0.97, -1) == 2
    assert acc.tolist() == [2.0, 0.5, 0.25]
    got = shared_epoch(mixed, [2, 2, 2], 1.0, 0.97, -1)
    assert got == former_epoch(mixed, [2, 2, 2], 1.0, 0.97, -1)
    assert got[1:] == (3, 2)


def test_sums_are_divided_by_the_supervised_batch_count():
    """Inherited from the reference: with --unsup_batch_ratio 2 the consistency figures are still per ITERATION."""
    got = shared_epoch(WITH_UNSUP, [2] * 4, 1.0, 0.97, -1)
    assert got == former_epoch(WITH_UNSUP, [2] * 4, 1.0, 0.97, -1)
    assert got[1:] == (4, 8)
    assert got[0][1] == 0.9375 / 4 and got[0][1] != 0.9375 / 8
    assert got[0][2] == 1.75 / 4


@pytest.mark.parametrize('name,checks_consistency,polls', NAN_POLICIES)
def test_nan_policy_of_each_trainer(name, checks_consistency, polls):
    # the policy the trainer hands to run_epochs, read off its call
    src = inspect.getsource(getattr(__import__(name), name))
    assert 'nan_checks_consistency={}'.format(checks_consistency) in src
    assert 'polls_step_nan={}'.format(polls) in src
    nan = float('nan')
    # the trainers' former tests: np.isnan(sup) for CutMix, np.isnan(sup) or np.isnan(consistency) for the other three
    for sup, cons in ((1.0, 0.5), (nan, 0.5), (1.0, nan), (nan, nan), (1.0, 0.0)):
        former = bool(np.isnan(sup) or np.isnan(cons)) if checks_consistency else bool(np.isnan(sup))
        assert tc.network_dead(np.float64(sup), np.float64(cons), checks_consistency) is former
    # ... on figures that went through the accumulator: a NaN consistency loss of one iteration
    means, _, _ = shared_epoch([_res(1.0, 0.5, 0.5), _res(1.0, nan, 0.5)], [1, 1], 1.0, 0.97, -1)
    assert means[0] == 1.0 and math.isnan(means[1])
    assert tc.network_dead(*means[:2], checks_consistency) is checks_consistency


class _Step(object):
    align_corners = True

    def __init__(self, results, dead_from=None):
        self.results, self.calls, self.dead_from = results, 0, dead_from

    def nan_detected(self):
        return self.dead_from is not None and self.calls >= self.dead_from

    def __call__(self, sup_x, sup_y, unsup, ramp_val=1.0):
        self.calls += 1
        return self.results[self.calls - 1]


class _Evaluator(object):
    """Stands in for evaluation.EvaluatorIoU (which histograms on the GPU): the per-class IoU is whatever evaluate() left."""
    reduced = 0

    def __init__(self, n_classes, fill_holes):
        self.iou = None

    def all_reduce(self):
        _Evaluator.reduced += 1

    def score(self):
        return self.iou


@pytest.mark.parametrize('name,checks_consistency,polls', NAN_POLICIES)
def test_run_epochs_log_lines_and_bails(name, checks_consistency, polls, monkeypatch, capsys):
    from cutmix_semisup_seg_amd import evaluation
    monkeypatch.setattr(evaluation, 'EvaluatorIoU', _Evaluator)
    data_parallel = name in ('train_seg_semisup_mask_mt', 'train_seg_semisup_vat_mt')
    img_per_s_of = (2, 1) if name == 'train_seg_semisup_mask_mt' else None
    net, tea = torch.nn.Identity(), torch.nn.Identity()

    def evaluate(evaluator):
        assert not tea.training
        evaluator.iou = np.array([0.5, 0.25])

    def run(step, rank=0, epochs=1):
        _Evaluator.reduced = 0
        capsys.readouterr()
        done = tc.run_epochs(step, lambda: (None, None, [None]), evaluate, net, tea, tea, (None, None), epochs, 2, False, -1,
                             0.97, 2, False, 'cpu', data_parallel=data_parallel, rank=rank,
                             nan_checks_consistency=checks_consistency, polls_step_nan=polls, img_per_s_of=img_per_s_of)
        return done, capsys.readouterr().out.splitlines()

    bail = 'NaN detected; network dead, bailing.'
    done, out = run(_Step([_res(1.5, 0.25, 0.5), _res(0.5, 0.25, 1.0)] * 2), epochs=2)
    assert done and out[0] == 'Training...' and net.training and _Evaluator.reduced == (2 if data_parallel else 0)
    assert len(out) == 1 + 2 * (3 if img_per_s_of else 2)
    took = out[1].split('took ')[1].split('s,')[0]
    assert out[1] == ('Epoch 1: took {}s, TRAIN clf loss=1.000000, consistency loss=0.250000, conf rate=75.000%, '
                      'VAL mIoU=37.500%'.format(took))
    assert out[2] == '-- 50.000%, 25.000%'
    if img_per_s_of:
        assert out[3].startswith('-- ') and out[3].endswith(' img/s (1 GPU)')
        assert out[4].startswith('Epoch 2: took ')
    else:
        assert out[3].startswith('Epoch 2: took ')
    # only the data-parallel trainers gate their prints on rank 0
    done, out = run(_Step([_res(1.5, 0.25, 0.5), _res(0.5, 0.25, 1.0)]), rank=1)
    assert done and (out == ['Training...'] if data_parallel else len(out) == 3)
    # a NaN supervised loss ends every trainer after the epoch's iterations, before the evaluation
    done, out = run(_Step([_res(float('nan'), 0.25, 0.5), _res(0.5, 0.25, 1.0)]))
    assert not done and out == ['Training...', bail]
    # a NaN consistency loss ends all but the CutMix trainer
    done, out = run(_Step([_res(1.0, float('nan'), 0.5), _res(0.5, 0.25, 1.0)]))
    assert done is (not checks_consistency)
    assert (out[1] == bail) if checks_consistency else ('consistency loss=nan' in out[1])
    # the step's own flag is asked before every iteration by the CutMix trainer alone: it ends the job one iteration late
    step = _Step([_res(1.5, 0.25, 0.5), _res(0.5, 0.25, 1.0)], dead_from=1)
    done, out = run(step)
    assert (done, step.calls, out[1] == bail) == ((False, 1, True) if polls else (True, 2, False))
