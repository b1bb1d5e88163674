"""
CPU-only checks of the class-threshold consistency:
  * the cases the GPU test shares (tests/_cthresh_refs.py) keep their margins at every pixel under every threshold vector, sit on
    the kernel routes they are there for, and their vectors do what they are there for
  * the fp64 restatement with a constant vector thr == tau IS _loss_refs.consistency(tau): scalars and gradient
  * KAPPA_Q is at least what the restatement's own formulas lose in fp32 on these inputs
  * the update arithmetic of the restatement on hand-made integer tables (tests/test_cthresh_hostcheck.py holds the header to it)
  * the command line of train_seg_semisup_classthresh_mt: the CutMix trainer's plus three options; its refusals, before the GPU
  * StepConfig() without class_thresh builds the ConsistencyConfig it built before
"""
import numpy as np
import pytest

import _cthresh_refs as R
import _loss_refs as L

ALL = R.CASES + [R.REFUSED]


# ------------------------------------------------------------------------------------------------------------ cases
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_case_margins_and_vectors(case):
    name, mode = case[0], case[1]
    C = R.geometry(name)[1]
    for vec in R.VECTORS:
        ref = R.reference(case, vec)
        print(R.case_id(case), vec, 'gap %.3g conf_margin %.3g share %.3f' % (ref['gap'], ref['conf_margin'], ref['pass_share']))
        assert ref['gap'] >= R.GAP and ref['conf_margin'] >= R.CONF
        thr = ref['thr']
        assert thr.dtype == np.float32 and thr.shape == (C,) and (thr >= 0).all() and (thr <= 1).all()
        if vec == 'one':
            assert (thr == 1.0).sum() == 1
            k = int(np.argmax(thr == 1.0))
            assert ref['table'][2 + C + k] > 0 and ref['table'][2 + 2 * C + k] == 0          # predicted, never passes
        if vec == 'floor':
            assert (thr == 0.0).sum() == 1
            k = int(np.argmax(thr == 0.0))
            assert ref['table'][2 + 2 * C + k] == ref['table'][2 + C + k] > 0                # always passes
        if name == 'one':
            continue            # 1 x 1 logits: two distinct teacher rows in all, nothing to be "about half" or unlike a scalar
        if vec == 'ascending':
            assert (np.diff(thr) > 0).all()                                                  # rising with the class index
        assert 0.15 <= ref['pass_share'] <= 0.85
        assert not ref['scalar_like']            # some passing pixel is less confident than some failing one: no scalar does this


@pytest.mark.parametrize('name', sorted(R.ROUTES))
def test_every_geometry_is_on_the_route_it_is_there_for(name):
    N, C, h, w, H, W, ac = R.geometry(name)
    f = L.tile_facts(C, h, w, H, W, ac, 3)
    for k, v in R.ROUTES[name].items():
        assert f[k] == v, (name, k, f[k], v)
    assert {c[0] for c in ALL} == set(R.ROUTES)
    # compile-time classes 2 / 5 / 19 / 21 and the run-time class count
    assert {R.geometry(c[0])[1] for c in R.CASES} >= {2, 5, 19, 21, 4, 3}
    assert {c[2] for c in R.CASES} == set(L.LOSS_FNS) and {c[1] for c in R.CASES} == {'mix', 'cut'}


@pytest.mark.parametrize('case', ALL, ids=R.case_id)
def test_kappa_q_of_every_case_is_below_the_constant(case):
    N, C, h, w, H, W, ac = R.geometry(case[0])
    k = R.kappa_q(R.inputs(case), H, W, ac, case[1])
    print(R.case_id(case), 'kappa_q %.3f' % k)
    assert k <= R.KAPPA_Q


# ------------------------------------------------------------------------------------------------------------ tie to _loss_refs
@pytest.mark.parametrize('case', [R.CASES[0], R.CASES[1], R.CASES[3], R.CASES[5], R.CASES[8]], ids=R.case_id)
@pytest.mark.parametrize('tau', [0.5, 0.9])
def test_constant_vector_is_the_scalar_threshold(case, tau):
    name, mode, fn, pp, given = case
    N, C, h, w, H, W, ac = R.geometry(name)
    i = R.inputs(case)
    thr = np.full(C, tau, dtype=np.float32)
    a = R.consistency(i, H, W, ac, mode, fn, thr, pp, R.RAMP, R.WEIGHT)
    b = L.consistency(i['ls'], i['l0'], i['l1'], H, W, ac, mode, fn, float(np.float32(tau)), pp, ranges=i['ranges'], mask=i['mask'],
                      invert=True, um0=i['um0'], um1=i.get('um1'), ramp=R.RAMP, weight=R.WEIGHT)
    assert a['scalars'] == b['scalars']
    assert np.array_equal(a['grad'], b['grad'])
    assert np.array_equal(L.grad_bound(a), L.grad_bound(b)) and L.scalar_bound(a) == L.scalar_bound(b)
    # and the table counts what the scalar rate counts, on the valid pixels
    assert sum(a['table'][2 + 2 * C:]) == int(((b['conf'] >= float(np.float32(tau))) & a['valid']).sum())


# ------------------------------------------------------------------------------------------------------------ update arithmetic
def test_update_first_step_from_one_over_c():
    C = 4
    state, thr = R.initial(C)
    assert state == [0.25] * 5 and [float(t) for t in thr] == [0.25] * 4
    one = 1 << 24
    table = [10, 9 * one, 7 * one, 2 * one, one, 0, 7, 2, 1, 0, 7, 2, 0, 0]
    s, t, tab, ep = R.update(state, thr, table, [0] * 9, C, True, 0.5, 0.0, 0.97)
    assert s[0] == 0.5 * 0.25 + 0.5 * 0.9
    assert s[1:] == [0.5 * 0.25 + 0.5 * p for p in (0.7, 0.2, 0.1, 0.0)]
    assert [float(v) for v in t] == [float(np.float32(s[0] * p / s[1])) for p in s[1:]]
    assert tab == [0] * 14 and ep == [10, 7, 2, 1, 0, 7, 2, 0, 0]


def test_update_with_no_valid_pixel_leaves_everything():
    C = 3
    state, thr = [0.6, 0.5, 0.3, 0.2], [np.float32(0.6), np.float32(0.36), np.float32(0.24)]
    s, t, tab, ep = R.update(state, thr, [0] * 11, [5, 1, 2, 3, 1, 1, 1], C, True, 0.9, 0.0, 0.97)
    assert s == state and t == thr and ep == [5, 1, 2, 3, 1, 1, 1] and tab == [0] * 11


def test_update_clamps_and_a_twice_attained_maximum():
    one = 1 << 24
    C = 2
    s, t, _, _ = R.update(*R.initial(C), [5, 5 * one, 5 * one, 0, 5, 0, 5, 0], [0] * 5, C, True, 0.0, 0.0, 0.97)
    assert s[0] == 1.0 and float(t[0]) == float(np.float32(0.97)) and float(t[1]) == 0.0                  # ceiling; floor 0
    s, t, _, _ = R.update(*R.initial(C), [5, 5 * one, 5 * one, 0, 5, 0, 5, 0], [0] * 5, C, True, 0.0, 0.3, 1.0)
    assert float(t[0]) == 1.0 and float(t[1]) == float(np.float32(0.3))                                   # ceiling 1; floor
    C = 4
    s, t, _, _ = R.update(*R.initial(C), [8, 6 * one, 3 * one, 3 * one, one, one, 4, 4, 0, 0, 2, 1, 0, 0], [0] * 9, C, True, 0.5, 0.0, 0.97)
    assert s[1] == s[2] == max(s[1:]) and t[0] == t[1] == np.float32(min(0.97, s[0])) and t[2] == t[3] < t[0]
    # static mode moves only the counters
    st, th = [0.25] * 5, [np.float32(v) for v in (0.9, 0.8, 0.7, 0.6)]
    s, t2, tab, ep = R.update(st, th, [8, 6 * one, 3 * one, 3 * one, one, one, 4, 4, 0, 0, 2, 1, 0, 0], [1] * 9, C, False, 0.5, 0.0, 0.97)
    assert s == st and t2 == th and tab == [0] * 14 and ep == [9, 5, 5, 1, 1, 3, 2, 1, 1]


# ------------------------------------------------------------------------------------------------------------ command line
def _table(command):
    return [(p.name, type(p.type).__name__, p.default, getattr(p, 'is_flag', False)) for p in command.params]


def test_option_table_is_the_cutmix_trainers_plus_three():
    import train_seg_semisup_mask_mt as cutmix
    import train_seg_semisup_classthresh_mt as ct
    base, got = _table(cutmix.experiment), _table(ct.experiment)
    assert got[:len(base)] == base                               # every shared option keeps its place, type and default
    assert got[len(base):] == [('class_thresh', 'StringParamType', 'freematch', False), ('thresh_ema', 'FloatParamType', None, False),
                               ('thresh_floor', 'FloatParamType', None, False)]
    assert ct.train_seg_semisup_classthresh_mt is not None


def _no_gpu(monkeypatch):
    import torch

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was touched')
    for name in ('is_available', 'current_device', 'set_device', 'init', '_lazy_init'):
        monkeypatch.setattr(torch.cuda, name, no_gpu)


REFUSALS = [
    (['--class_thresh', '0.5,abc'], '--class_thresh'),
    (['--class_thresh', '0.5,,0.5'], '--class_thresh'),
    (['--class_thresh', '0.5,0.0,0.7'], '--class_thresh'),                      # not in (0, 1]
    (['--class_thresh', '0.5,1.5,0.7'], '--class_thresh'),
    (['--class_thresh', '0.5,0.6', '--synthetic_n_classes', '3'], '--class_thresh'),          # two numbers for three classes
    (['--thresh_floor', '0.98'], '--thresh_floor'),                             # above the ceiling (--conf_thresh 0.97)
    (['--thresh_floor', '0.5', '--conf_thresh', '0.4'], '--thresh_floor'),
    (['--thresh_floor', '-0.1'], '--thresh_floor'),
    (['--thresh_ema', '1.0'], '--thresh_ema'),
    (['--thresh_ema', '-0.5'], '--thresh_ema'),
    (['--conf_thresh', '0'], '--conf_thresh'),
    (['--conf_thresh', '1.5'], '--conf_thresh'),
    (['--class_thresh', '0.5,0.6,0.7', '--synthetic_n_classes', '3', '--thresh_ema', '0.9'], '--thresh_ema'),
    (['--class_thresh', '0.5,0.6,0.7', '--synthetic_n_classes', '3', '--thresh_floor', '0.1'], '--thresh_floor'),
]


@pytest.mark.parametrize('extra,names', REFUSALS, ids=lambda v: ' '.join(v) if isinstance(v, list) else None)
def test_command_refusals_come_before_the_gpu(tmp_path, monkeypatch, extra, names):
    from click.testing import CliRunner
    import train_seg_semisup_classthresh_mt as ct
    _no_gpu(monkeypatch)
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    res = CliRunner().invoke(ct.experiment, ['--synthetic', '--crop_size', '33,33'] + extra)
    assert res.exit_code != 0 and isinstance(res.exception, ValueError), (res.output, res.exception)
    assert names in str(res.exception), res.exception


def test_more_than_one_process_is_refused_before_the_gpu(tmp_path, monkeypatch):
    from click.testing import CliRunner
    import train_seg_semisup_classthresh_mt as ct
    _no_gpu(monkeypatch)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv('WORLD_SIZE', '2')
    res = CliRunner().invoke(ct.experiment, ['--synthetic', '--crop_size', '33,33'])
    assert res.exit_code != 0 and isinstance(res.exception, ValueError) and 'one process' in str(res.exception)


def test_checked_options_and_the_report_lines():
    from cutmix_semisup_seg_amd.train_seg_semisup_classthresh_mt import checked_options, format_report
    assert checked_options('freematch', None, None, 0.97) == ('freematch', 0.999, 0.0)
    assert checked_options('FreeMatch', 0.5, 0.2, 1.0) == ('freematch', 0.5, 0.2)
    assert checked_options('0.5, 1.0,0.25', None, None, 0.97, 3) == ([0.5, 1.0, 0.25], 0.0, 0.0)
    with pytest.raises(ValueError, match='--class_thresh'):
        checked_options('0.5,0.6', None, None, 0.97, 3)
    lines = format_report(dict(thr=np.array([0.812, 0.455, 0.1], np.float32), tau=0.812, pass_rate=[0.712, 0.125, None]))
    assert lines == ['-- class thresholds tau=0.812: 0.812, 0.455, 0.100', '-- class pass rate 71.2%, 12.5%, -']


# ------------------------------------------------------------------------------------------------------------ host layers
def test_step_config_without_class_thresh_is_what_it_was():
    from cutmix_semisup_seg_amd import ops
    from cutmix_semisup_seg_amd.step import StepConfig
    cfg = StepConfig(mask_mode='zero', cons_loss_fn='kld', conf_thresh=0.6, conf_per_pixel=True, invert=False)
    assert cfg.class_thresh is None and cfg.cons.class_thresh is None
    want = ops.ConsistencyConfig(mode='cut', loss_fn='kld', conf_thresh=0.6, conf_per_pixel=True, invert=False)
    assert vars(cfg.cons) == vars(want)
    assert vars(StepConfig().cons) == vars(ops.ConsistencyConfig())
    assert sorted(vars(want)) == ['align_corners', 'class_thresh', 'conf_per_pixel', 'conf_thresh', 'invert', 'loss_fn', 'mode']
    with pytest.raises(TypeError):
        ops.ConsistencyConfig(class_thresh=[0.5, 0.5])                          # a ClassThresholds, not a list
    with pytest.raises(RuntimeError, match='GPU only'):
        ops.ClassThresholds(3, 'cpu')


def test_parse_class_thresh():
    from cutmix_semisup_seg_amd.ops import parse_class_thresh
    assert parse_class_thresh('freematch') == 'freematch' and parse_class_thresh(' 0.5 ,1 ') == [0.5, 1.0]
    for bad in ('', 'free', '0.5;0.6', '0,0.5', 'nan,0.5', '1.01'):
        with pytest.raises(ValueError):
            parse_class_thresh(bad)
    with pytest.raises(ValueError, match='3 classes'):
        parse_class_thresh('0.5,0.6', 3)
