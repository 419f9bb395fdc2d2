"""tests/child_harness.py and the verdict of tests/gpu_children.py without a
GPU: the job loop's three outcomes, the start-up check, the refusal check and
the float64 guard layout on the 'cpu' device, and the latch with
subprocess.run replaced by prepared results (no child is started and none
dies; the real suite's latch and cache are put back afterwards)."""
import json
import subprocess

import numpy as np
import pytest

from tests import child_harness as ch
from tests import gpu_children as gc
from tests import spmm_driver as drv

F32 = drv.PRECISIONS['f32']


# ---------------------------------------------------------------------------
# run_jobs
# ---------------------------------------------------------------------------

def _run(capsys, jobs, **kwargs):
    status = ch.run_jobs(jobs, {'env': 'e', 'prec': 'p'}, **kwargs)
    out = capsys.readouterr()
    return status, [json.loads(raw) for raw in out.out.splitlines()], out.err


def _raiser(exc):
    def job():
        raise exc
    return job


def test_run_jobs_all_ok(capsys):
    status, lines, _ = _run(capsys, [
        ('a', lambda: dict(x=1)),
        ('b', lambda: dict(y=2.5), dict(matrix='std', k=8, other='dropped')),
        ('c', lambda: {})])
    assert status == 0
    assert [ln['case'] for ln in lines] == ['a', 'b', 'c']
    for ln in lines:
        assert ln['ok'] is True and ln['env'] == 'e' and ln['prec'] == 'p'
        assert ln['ms'] >= 0 and 'error' not in ln and 'errored' not in ln
    assert lines[0]['x'] == 1 and lines[1]['y'] == 2.5
    assert lines[1]['matrix'] == 'std' and lines[1]['k'] == 8
    assert 'other' not in lines[1]


def test_run_jobs_stops_at_a_failed_case(capsys):
    ran = []
    status, lines, _ = _run(capsys, [
        ('a', lambda: {}),
        ('b', _raiser(ch.Mismatch('x' * 3000))),
        ('c', lambda: ran.append('c') or {})])
    assert status == 1 and not ran
    assert [ln['case'] for ln in lines] == ['a', 'b']
    assert lines[1]['ok'] is False and lines[1]['error'] == 'x' * 2000
    assert 'errored' not in lines[1] and 'ms' in lines[1]


def test_run_jobs_reports_an_errored_child(capsys):
    ran = []
    status, lines, err = _run(capsys, [
        ('a', lambda: {}),
        ('b', _raiser(RuntimeError('HIP error: an illegal memory access'))),
        ('c', lambda: ran.append('c') or {})])
    assert status == ch.EXIT_ERRORED and not ran
    assert ch.EXIT_ERRORED not in (0, 1) + gc.FATAL_STATUS
    assert [ln['case'] for ln in lines] == ['a', 'b']
    assert lines[1]['ok'] is False and lines[1]['errored'] is True
    assert lines[1]['error'] == \
        'RuntimeError: HIP error: an illegal memory access'
    assert 'Traceback' in err and 'RuntimeError' in err


def test_run_jobs_failed_parameter(capsys):
    jobs = [('a', _raiser(MemoryError('out of memory')))]
    status, lines, _ = _run(capsys, jobs)
    assert status == ch.EXIT_ERRORED and lines[0]['errored'] is True
    status, lines, _ = _run(capsys, jobs,
                            failed=(AssertionError, MemoryError))
    assert status == 1 and 'errored' not in lines[0]
    assert lines[0]['error'] == 'out of memory'


def test_run_jobs_before_and_after(capsys):
    calls = []

    def after(line):
        calls.append(('after', line['case'], line['ok']))
        line['peak'] = len(calls)

    status, lines, _ = _run(
        capsys, [('a', lambda: calls.append(('job', 'a')) or {}),
                 ('b', lambda: calls.append(('job', 'b')) or {})],
        before=lambda name: calls.append(('before', name)), after=after)
    assert status == 0
    assert calls == [('before', 'a'), ('job', 'a'), ('after', 'a', True),
                     ('before', 'b'), ('job', 'b'), ('after', 'b', True)]
    assert [ln['peak'] for ln in lines] == [3, 6]


# ---------------------------------------------------------------------------
# started_with
# ---------------------------------------------------------------------------

NAMES = ('ARROW_T_A', 'ARROW_T_B', 'ARROW_T_C')


def test_started_with(monkeypatch):
    for var in NAMES:
        monkeypatch.delenv(var, raising=False)
    ch.started_with(NAMES, {})
    monkeypatch.setenv('ARROW_T_A', '1')
    monkeypatch.setenv('ARROW_T_B', '0')
    ch.started_with(NAMES, {'ARROW_T_A': '1', 'ARROW_T_B': '0'})
    with pytest.raises(AssertionError, match='ARROW_T_C'):      # missing
        ch.started_with(NAMES, {'ARROW_T_A': '1', 'ARROW_T_B': '0',
                                'ARROW_T_C': '2'})
    with pytest.raises(AssertionError, match='ARROW_T_B'):      # one extra
        ch.started_with(NAMES, {'ARROW_T_A': '1'})
    with pytest.raises(AssertionError, match='ARROW_T_A'):      # wrong value
        ch.started_with(NAMES, {'ARROW_T_A': '0', 'ARROW_T_B': '0'})


# ---------------------------------------------------------------------------
# refused
# ---------------------------------------------------------------------------

def _buffers():
    bits = F32.bits(np.arange(24, dtype=np.float32).reshape(3, 8))
    cbuf, cv = ch.guarded(F32, bits, F32.c_guard, 'cpu')
    abuf, av = ch.guarded_f64([3.5, -2.25], 8, 'cpu')
    return cbuf, cv, abuf, av, {
        'C': (cbuf, cv, F32.c_guard, bits),
        'acc': (abuf, av, ch.F64_GUARD, [3.5, -2.25])}


def test_refused_passes():
    *_, unchanged = _buffers()
    ch.refused(lambda: (-3, "R is NULL but gamma is 2"),
               ('R is NULL', 'gamma'), unchanged)
    ch.refused(lambda: (-1, "all NULL"), ('all NULL',), {})


def test_refused_raises():
    cbuf, cv, abuf, av, unchanged = _buffers()
    with pytest.raises(ch.Mismatch, match='misuse accepted'):
        ch.refused(lambda: (0, "R is NULL"), ('R is NULL',), unchanged)
    with pytest.raises(ch.Mismatch, match='does not name'):
        ch.refused(lambda: (-1, "R is NULL"), ('R is NULL', 'gamma'),
                   unchanged)
    cv[5] ^= 1                              # one element of the view
    with pytest.raises(ch.Mismatch, match='C was written by a refused call'):
        ch.refused(lambda: (-1, "no"), ('no',), unchanged)
    cv[5] ^= 1
    ch.refused(lambda: (-1, "no"), ('no',), unchanged)
    for buf, at, name in ((cbuf, ch.PAD - 1, 'C'), (cbuf, -ch.PAD, 'C'),
                          (abuf, 7, 'acc'), (abuf, 10, 'acc')):
        keep = buf[at].clone()              # one guard word
        buf[at] = 0
        with pytest.raises(ch.Mismatch, match=f'{name} was written'):
            ch.refused(lambda: (-1, "no"), ('no',), unchanged)
        buf[at] = keep
    av[1] = 0.0                             # one accumulator
    with pytest.raises(ch.Mismatch, match='acc was written'):
        ch.refused(lambda: (-1, "no"), ('no',), unchanged)


# ---------------------------------------------------------------------------
# the float64 guard layout
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('pad', [8, 16])
def test_f64_guard_layout(pad):
    values = np.arange(5, dtype=np.float64) + 0.5
    buf, view = ch.guarded_f64(values, pad, 'cpu')
    assert buf.numel() == 5 + 2 * pad and view.numel() == 5
    assert view.data_ptr() - buf.data_ptr() == pad * 8
    assert (buf[:pad] == ch.F64_GUARD).all()
    assert (buf[-pad:] == ch.F64_GUARD).all()
    assert (view.numpy() == values).all()
    assert ch.f64_guards_intact(buf)
    other, _ = ch.guarded_f64(values, pad, 'cpu')
    for at in (0, pad - 1, pad + 5, 5 + 2 * pad - 1):   # both ends of each
        buf, _ = ch.guarded_f64(values, pad, 'cpu')
        buf[at] = 0
        assert not ch.f64_guards_intact(buf)
        assert not ch.f64_guards_intact(other, buf)
    buf, view = ch.guarded_f64(values, pad, 'cpu')
    view[:] = 0                             # the view is not a guard
    assert ch.f64_guards_intact(buf)


# ---------------------------------------------------------------------------
# run_child and child_ok
# ---------------------------------------------------------------------------

def _stdout(*lines):
    return ''.join(json.dumps(ln) + '\n' for ln in lines)


OK_LINES = _stdout(dict(case='a', ok=True, ms=1.0),
                   dict(case='b', ok=True, ms=1.0))


@pytest.fixture
def children(monkeypatch):
    """gpu_children with an open latch and an empty cache of its own, and
    subprocess.run answering from `script`: a list of CompletedProcess
    arguments (returncode, stdout, stderr) or exceptions, one per start."""
    monkeypatch.setattr(gc, '_stopped', None)
    monkeypatch.setattr(gc, '_results', {})
    script, started = [], []

    def fake_run(argv, **kwargs):
        started.append(argv)
        answer = script.pop(0)
        if isinstance(answer, Exception):
            raise answer
        return subprocess.CompletedProcess(argv, *answer)
    monkeypatch.setattr(gc.subprocess, 'run', fake_run)
    return script, started


def _child_ok(expected, key='k'):
    return gc.child_ok(key, ['driver.py'], {}, (), 10, 'the child', expected)


def test_child_ok_passes_and_is_cached(children):
    script, started = children
    script.append((0, OK_LINES, ''))
    assert set(_child_ok(['a', 'b'])) == {'a', 'b'}
    assert set(_child_ok(['a'])) == {'a', 'b'}          # script is empty
    assert len(started) == 1
    script.append((0, OK_LINES, ''))
    _child_ok(['a'], key='another')
    assert len(started) == 2


def test_child_ok_missing_name(children):
    children[0].append((0, OK_LINES, ''))
    with pytest.raises(AssertionError, match=r"cases not run: \['c'\]"):
        _child_ok(['a', 'b', 'c'])


def test_child_ok_bad_line(children):
    bad = dict(case='b', ok=False, error='differs from the reference')
    children[0].append((1, _stdout(dict(case='a', ok=True), bad), 'tail'))
    with pytest.raises(AssertionError) as e:
        _child_ok(['a', 'b'])
    assert str(bad) in str(e.value)
    assert gc._stopped is None              # a failed case does not latch
    children[0].append((0, OK_LINES, ''))
    _child_ok(['a'], key='next')


def test_child_ok_nonzero_status(children):
    children[0].append((1, OK_LINES, 'Traceback: the tail'))
    with pytest.raises(AssertionError, match='exit status 1\nTraceback'):
        _child_ok(['a'])
    assert gc._stopped is None


def _latched(children, match):
    with pytest.raises(pytest.fail.Exception, match=match):
        gc.run_child(['driver.py'], {}, (), 10, 'the child')
    started = len(children[1])
    for call in (lambda: gc.run_child(['driver.py'], {}, (), 10, 'next'),
                 lambda: _child_ok(['a']), gc.fail_if_stopped, gc.need_gpu):
        with pytest.raises(pytest.fail.Exception, match='not started: '):
            call()
    assert len(children[1]) == started      # nothing more was started


def test_errored_child_latches(children, monkeypatch):
    monkeypatch.setattr(gc.torch.cuda, 'is_available', lambda: True)
    line = dict(case='b', ok=False, errored=True,
                error='RuntimeError: HIP error: an illegal memory access')
    children[0].append((ch.EXIT_ERRORED,
                        _stdout(dict(case='a', ok=True), line), 'Traceback'))
    _latched(children, "case 'b' errored: RuntimeError: HIP error")


@pytest.mark.parametrize('status', gc.FATAL_STATUS + (-11,))
def test_fatal_status_latches(children, monkeypatch, status):
    monkeypatch.setattr(gc.torch.cuda, 'is_available', lambda: True)
    children[0].append((status, OK_LINES, ''))
    _latched(children, f'ended with status {status} after 2 cases')


def test_time_limit_latches(children, monkeypatch):
    monkeypatch.setattr(gc.torch.cuda, 'is_available', lambda: True)
    children[0].append(subprocess.TimeoutExpired(['driver.py'], 10))
    _latched(children, 'hit its 10s limit')


def test_need_gpu(children, monkeypatch):
    monkeypatch.setattr(gc.torch.cuda, 'is_available', lambda: False)
    with pytest.raises(pytest.skip.Exception):
        gc.need_gpu()
    monkeypatch.setattr(gc.torch.cuda, 'is_available', lambda: True)
    for var in gc.ENGINE_VARS:
        monkeypatch.delenv(var, raising=False)
    gc.need_gpu()
    monkeypatch.setenv('ARROW_FOLD', '1')
    with pytest.raises(AssertionError, match='ARROW_FOLD'):
        gc.need_gpu()
    gc.need_gpu(clean=())
