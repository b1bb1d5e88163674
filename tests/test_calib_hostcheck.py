"""
CPU-only: csrc/calib_math.hpp -- the functions the kernel of csrc/calib.hip is made of -- driven on the host by a small program of
its own (tests/hostcheck_calib) over every case of the GPU test, against the fp64 restatement (tests/_calib_refs.py) under
its acceptance rule; the bit-for-bit claims of the definition (the confidence of the consistency kernels, the cross entropy of the
supervised loss, the prediction of the vote); every descriptor refusal; and the same stand-alone program once more under the host's
address and undefined-behaviour sanitizers.
"""
import numpy as np
import pytest

import _hostcheck
import _calib_refs as R


@pytest.fixture(scope='module')
def host():
    exe = _hostcheck.build('hostcheck_calib')

    def run(inp, program=exe, **kw):
        return R.hostcheck_run(program, inp, **kw)
    return run


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_header_on_the_host_vs_restatement(host, name):
    inp, ref = R.case(name)
    got = host(inp)
    e_conf, e_brier, e_nll = R.pixel_errors(got, ref)
    print(name, 'max |fp32 - fp64| on the host: conf {:.3g} squared error {:.3g} nll {:.3g}; ambiguous {} of {}'.format(
        e_conf, e_brier, e_nll, ref['ambiguous'], int(ref['scores'][0])))
    # the bounds are twice the largest figure printed here (the record is in _calib_refs.py): every pixel is inside them
    assert e_conf <= R.B_CONF and e_brier <= R.B_BRIER and e_nll <= R.B_NLL
    R.accept(got, ref)


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_bit_for_bit_claims(host, name):
    """k == 1, T == 1: conf is consistency_pixel_fwd's and nll ce_pixel_fwd's; T == 1 or k == 1: pred is the vote's"""
    inp, _ = R.case(name)
    claims = host(inp)['claims']
    k, t0 = inp['k'], float(inp['temps'][0])
    want = [0 if k == 1 and t0 == 1.0 else -1] * 2 + [0 if (k == 1 or t0 == 1.0) else -1]
    assert claims.tolist() == want


def test_the_claims_are_checked_somewhere():
    names = [n for n in R.CASES if R.CASES[n]['k'] == 1 and R.CASES[n]['temps'][0] == 1.0 and not R.CASES[n]['ignore_all']]
    assert len(names) >= 4 and any(R.CASES[n]['k'] >= 2 and R.CASES[n]['temps'][0] == 1.0 for n in R.CASES)


def test_host_driver_refuses_what_the_library_refuses(host):
    inp, _ = R.case('k2_c19_T1')
    e = inp['edges']
    for over in (dict(n=0), dict(c=0), dict(c=65), dict(H=0), dict(W=-1), dict(k=0), dict(k=17), dict(label_dtype=7),
                 dict(nb=0), dict(nb=49), dict(edges=np.r_[e, e[-1]]), dict(nt=0), dict(nt=9),
                 dict(edges=e[::-1]), dict(edges=np.r_[e[:3], e[2:]]), dict(edges=np.r_[0.0, e[1:]]), dict(edges=np.r_[e[:-1], 1.0]),
                 dict(edges=np.r_[e[:-1], np.nan]), dict(edges=np.r_[-0.1, e[1:]]),
                 dict(temps=[0.0]), dict(temps=[-1.0]), dict(temps=[np.nan]), dict(temps=[np.inf]), dict(temps=[1.0, 0.0]),
                 dict(null=('hist',)), dict(null=('scores',)), dict(null=('labels',)), dict(null=('labels', 'cm')),
                 dict(null=('edges',)), dict(null=('temps',)), dict(null=('cm', 'pred_out'))):
        host(inp, expect_code=2, **over)
    # and accepts what it should: no cm, no pred_out
    got = host(inp, null=('cm',))
    assert not got['cm'].any()
    host(inp, null=('pred_out',))


def test_more_than_48_bins_is_refused(host):
    inp, _ = R.case('k2_c19_T1')
    host(inp, expect_code=2, edges=np.arange(1, 49) / 49.0)
    host(inp, edges=np.arange(1, 48) / 48.0)


def test_stand_alone_under_the_host_sanitizers(host):
    """The same program with its own main, built with -fsanitize=address,undefined, as a process of its own."""
    exe = _hostcheck.build('hostcheck_calib', sanitize=True)
    for name in ('k1_c2_T1', 'k1_c21_T0.5', 'k2_c19_nt8', 'k1_c19_nt8_i64', 'lds_worst_k16_c64_nb48', 'nb1_k2_c19', 'one_pixel_k1',
                 'one_pixel_k2', 'all_ignored_k5', 'hot_k5_c64'):
        inp, ref = R.case(name)
        R.accept(host(inp, program=exe), ref)
    inp, _ = R.case('k2_c19_T1')
    host(inp, program=exe, expect_code=2, nb=0)
    host(inp, program=exe, expect_code=2, null=('hist',))
