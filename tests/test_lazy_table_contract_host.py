"""The lazy-table check (csrc/step_state.h: make_lazy), the same for each of the six entries that take a table, without a GPU: through
_lib.call with made-up addresses -- the check comes before any launch and before the entry's n == 0 return, so nothing is dereferenced.

The conditions: lo >= 0, rows >= 0, rowlen > 0, rowlen % 4 == 0, lo % 4 == 0, lo <= n and rows <= (n - lo) / rowlen -- no product that
can wrap.  Before the entries shared one check, the Adam and norm entries (mmvid_adam_step_rows, mmvid_adam_step_guarded,
mmvid_grad_sqnorm_rows) tested lo + rows * rowlen <= n and accepted the three tables below whose product wraps, and
mmvid_grad_sqnorm_rows returned at n == 0 before it looked at the table at all: on that code this file fails on exactly those rows."""
import ctypes

import pytest

V = ctypes.c_void_p
A, B, C, D, E, FLAGS = (V(k << 20) for k in range(1, 7))
TABLES = [V(k << 20) for k in range(7, 10)]
REST = [V(k << 20) for k in range(10, 17)]  # count_dev, the partials, the ring and its headers


def _sqnorm(n, table, skip):
    return ('mmvid_grad_sqnorm_rows', A, n, B, C, *table, None)


def _adam(n, table, skip):
    return ('mmvid_adam_step_rows', A, B, C, D, None, n, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, 1, None, 1.0, None, 1.0, *table, None)


def _adam_guarded(n, table, skip):
    return ('mmvid_adam_step_guarded', *_adam(n, table, skip)[1:-1], skip, None)


def _ema(n, table, skip):
    return ('mmvid_ema_update', A, B, n, 0.9, 0, 1, None, *table, None)


def _ema_guarded(n, table, skip):
    return ('mmvid_ema_update_guarded', *_ema(n, table, skip)[1:-1], skip, None)


def _segment_stats(n, table, skip):
    return ('mmvid_segment_stats', A, B, C, D, n, *TABLES, 1, 1, 1e-3, None, 0.9, 0.999, 1e-8, 1, None, *table, skip, 1, 1, *REST, None)


ENTRIES = {'mmvid_grad_sqnorm_rows': _sqnorm, 'mmvid_adam_step_rows': _adam, 'mmvid_adam_step_guarded': _adam_guarded,
           'mmvid_ema_update': _ema, 'mmvid_ema_update_guarded': _ema_guarded, 'mmvid_segment_stats': _segment_stats}

# (what, lo, rows, rowlen, the buffer lengths n at which it is given)
REFUSED = [
    ('lo % 4 != 0', 6, 5, 12, (1000, 0)),
    ('lo < 0', -4, 5, 12, (1000, 0)),
    ('rowlen % 4 != 0', 8, 5, 10, (1000, 0)),
    ('rowlen == 0', 8, 5, 0, (1000, 0)),
    ('rows < 0', 8, -1, 12, (1000, 0)),
    ('a table reaching past n', 8, 5, 12, (67, )),
    ('a table of no rows that starts past n', 1004, 0, 4, (1000, 0)),
    ('rows * rowlen wraps to 0', 0, 1 << 62, 4, (1000, 0)),
    ('rows * rowlen wraps to 0 (rowlen 8)', 0, 1 << 61, 8, (1000, 0)),
    ('rows * rowlen wraps to 4', 8, (1 << 62) + 1, 4, (1000, 0)),
    ('a table of five rows in an empty buffer', 0, 5, 4, (0, )),
]


@pytest.mark.parametrize('entry', list(ENTRIES))
def test_entry_refuses_a_bad_lazy_table(entry):
    from mmvid_amd import _lib
    for what, lo, rows, rowlen, ns in REFUSED:
        for n in ns:
            with pytest.raises(_lib.MMVIDError, match='lazy'):
                _lib.call(*ENTRIES[entry](n, (FLAGS, lo, rows, rowlen), E))
                pytest.fail(f'{entry}: {what} at n = {n}: accepted')


@pytest.mark.parametrize('entry', list(ENTRIES))
def test_entry_accepts_no_table_and_an_empty_table(entry):
    """At n = 0 only: nothing is launched, with or without a GPU."""
    from mmvid_amd import _lib
    for table in ((None, 0, 0, 0), (FLAGS, 0, 0, 4)):
        for skip in (E, None):
            _lib.call(*ENTRIES[entry](0, table, skip))
