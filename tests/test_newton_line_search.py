"""CPU: the one line search of the Laplace mode finding (newton_line_search, csrc/laplace_newton.h), which every
driver calls, follows the reference's rules.

GPB_TestNewtonLineSearch feeds it a scripted sequence of trial objectives. The expectation is an independent
restatement of the reference's backtracking loop (likelihoods.h:1910-1928) and CheckConvergenceModeFinding
(:11820-11870, without the continue-after-Fisher branch no supported likelihood takes): a trial is rejected when it
is below obj + c_armijo lr grad_dot_direction (strict <), NaN or Inf, each rejection halves lr, the last trial is
kept when none is accepted; at it == 0 the step terminates on |change| < delta |obj|, later on change < delta |obj|.
Every learning rate is a power of two and is compared exactly; the slopes are powers of two as well, so that
c_armijo lr slope is c_armijo scaled exactly and the threshold does not depend on how the sum is rounded.
"""
import ctypes
import math

import numpy as np
import pytest

C_ARMIJO = 1e-4      # c_armijo_ (likelihoods.h:12737)
MAX_SHRINK = 20      # max_number_lr_shrinkage_steps_newton_ (:12725)
DELTA = 1e-8         # delta_conv_mode_finding_ (:12723)
NAN, INF = float("nan"), float("inf")


def restatement(it, obj, gdd, delta, max_shrink, objs):
    lr, new, lams = 1., obj, []
    for ih in range(max_shrink):
        new = objs[ih]
        lams.append(lr)
        if new < obj + C_ARMIJO * lr * gdd or math.isnan(new) or math.isinf(new):
            lr *= 0.5
        else:
            break
    bad = math.isnan(new) or math.isinf(new)
    terminate = False
    if not bad:
        change = new - obj
        terminate = (abs(change) if it == 0 else change) < delta * abs(obj)
    return new, lams[-1], len(lams), terminate, bad, lams


def library(it, obj, gdd, delta, max_shrink, objs):
    from gpboost_amd import basic
    D = ctypes.POINTER(ctypes.c_double)
    t = np.ascontiguousarray(objs, dtype=np.float64)
    out = np.full(5 + len(t), -7.0)
    ret = basic.lib().GPB_TestNewtonLineSearch(
        ctypes.c_int(it), ctypes.c_double(obj), ctypes.c_double(gdd), ctypes.c_double(delta), ctypes.c_int(max_shrink),
        t.ctypes.data_as(D), ctypes.c_int(len(t)), out.ctypes.data_as(D))
    assert ret == 0
    used = int(out[2])
    assert out[2] == used and np.all(np.isnan(out[5 + used:]))     # trials not run leave NaN
    return out[0], out[1], used, bool(out[3]), bool(out[4]), out[5:5 + used].tolist()


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def check(it, obj, gdd, max_shrink, objs, delta=DELTA):
    want = restatement(it, obj, gdd, delta, max_shrink, objs)
    got = library(it, obj, gdd, delta, max_shrink, objs)
    assert same(got[0], want[0]) and got[1:] == want[1:], (got, want)
    return got


def test_accepted_at_full_step():
    new, lam, used, term, bad, lams = check(1, -100., 8., MAX_SHRINK, [-90.])
    assert (new, lam, used, term, bad, lams) == (-90., 1., 1, False, False, [1.])


def test_accepted_at_the_fourth_halving():
    new, lam, used, term, bad, lams = check(1, -100., 8., MAX_SHRINK, [-200., -150., -120., -101., -99.])
    assert new == -99. and lam == 2. ** -4 and used == 5 and not term and not bad
    assert lams == [2. ** -k for k in range(5)]


def test_trial_equal_to_the_armijo_threshold_is_accepted():
    obj, gdd = -100., 8.
    threshold = obj + C_ARMIJO * 1. * gdd
    assert threshold > obj
    new, lam, used, _, _, _ = check(1, obj, gdd, MAX_SHRINK, [threshold])
    assert new == threshold and lam == 1. and used == 1             # strict <: equality is no rejection
    below = np.nextafter(threshold, -INF)
    _, lam, used, _, _, _ = check(1, obj, gdd, MAX_SHRINK, [below, -99.])
    assert lam == 0.5 and used == 2                                 # one ulp below is rejected


@pytest.mark.parametrize("it, terminates", [(0, False), (1, True)])
def test_no_trial_accepted_keeps_the_last(it, terminates):
    new, lam, used, term, bad, lams = check(it, -100., 8., MAX_SHRINK, [-200.] * MAX_SHRINK)
    assert new == -200. and lam == 2. ** -19 and used == MAX_SHRINK and not bad
    assert lams == [2. ** -k for k in range(MAX_SHRINK)]
    assert term is terminates          # a decrease: the signed rule of it > 0 stops, the absolute rule of it == 0 does not


def test_nan_then_inf_then_acceptable():
    new, lam, used, term, bad, lams = check(2, -100., 8., MAX_SHRINK, [NAN, INF, -95.])
    assert new == -95. and lam == 0.25 and used == 3 and not term and not bad and lams == [1., 0.5, 0.25]


@pytest.mark.parametrize("it", [0, 3])
def test_all_nan(it):
    new, lam, used, term, bad, _ = check(it, -100., 8., MAX_SHRINK, [NAN] * MAX_SHRINK)
    assert math.isnan(new) and lam == 2. ** -19 and used == MAX_SHRINK and bad and not term


def test_one_trial_allowed():
    """The latent Gaussian path passes max_shrink = 1: one trial, kept whatever it is (a second would be an error
    of the scripted sequence)."""
    new, lam, used, term, bad, lams = check(0, -100., 0., 1, [-200.])
    assert (new, lam, used, term, bad, lams) == (-200., 1., 1, False, False, [1.])


@pytest.mark.parametrize("it, terminates", [(0, False), (1, True)])
def test_tiny_decrease(it, terminates):
    """A decrease of 1e-3 at |obj| = 100 is above delta |obj| = 1e-6 in size: only the signed rule terminates."""
    new, _, used, term, bad, _ = check(it, -100., 0., MAX_SHRINK, [-100. - 1e-3] * MAX_SHRINK)
    assert new == -100. - 1e-3 and used == MAX_SHRINK and not bad and term is terminates
