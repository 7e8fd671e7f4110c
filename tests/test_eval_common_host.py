"""CPU check of the read-back cursor the evaluators' ``results()`` share (psd/eval_common.TableCursor): ``take``,
``take_pair`` and ``rest`` walk a hand-made array in order, and a request past the end raises.  No kernel is launched."""
import numpy as np
import pytest


def test_cursor_walks_the_array_in_order_and_refuses_an_overrun():
    from waveformml_amd.psd.eval_common import TableCursor
    host = np.arange(20, dtype=np.int64)
    cur = TableCursor(host)
    assert cur.take(2).tolist() == [0, 1]
    assert cur.take((2, 3)).tolist() == [[2, 3, 4], [5, 6, 7]]
    n, s = cur.take_pair((2, 2))                       # the count table, then its sum table
    assert n.tolist() == [[8, 9], [10, 11]] and s.tolist() == [[12, 13], [14, 15]]
    with pytest.raises(ValueError, match="TableCursor"):
        cur.take((5,))
    assert cur.at == 16                                # a refused request moves nothing
    assert cur.rest().tolist() == [16, 17, 18, 19]
    assert cur.rest().size == 0 and cur.take(0).size == 0
    with pytest.raises(ValueError, match="TableCursor"):
        cur.take(1)
