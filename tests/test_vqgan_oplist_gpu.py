"""`mmvid_vqgan_run` checks the whole op list before it enqueues the first op (csrc/vqgan.hip: mmvid_vqgan_check)."""
import ctypes

import pytest
import torch

from mmvid_amd import _lib, ops, vqgan_plan as P

pytestmark = pytest.mark.gpu


def test_refused_list_enqueues_nothing():
    """A valid IMG2NHWC8 op followed by a record the checker refuses, run directly (graph cache off): the call raises, the arena the
    first op would have written is untouched, and no sequence was counted as run.  Before the checker the first op had been launched
    when the error came back."""
    dev = torch.device('cuda', 0)
    img = torch.rand(1, 3, 16, 16, device=dev)
    arena = torch.full((16 * 16 * 8 * 2, ), 0xA5, device=dev, dtype=torch.uint8)  # exactly the bf16 [1,16,16,8] the first op writes
    arr = (_lib.VqganOp * 2)()
    for o in arr:
        o.in0 = o.in1 = o.in2 = o.out_bf16 = o.out_f32 = o.scratch = -1
    arr[0].op, arr[0].N, arr[0].H, arr[0].W, arr[0].C, arr[0].out_bf16, arr[0].ext_in = P._Planner.OP_IMG, 1, 16, 16, 3, 0, img.data_ptr()
    arr[1].op, arr[1].flags = P._Planner.OP_CAST, P.STRICT | P.SPLIT
    assert _lib.load().mmvid_vqgan_check(arr, 1) == 0  # the first op alone is a valid list

    def stats():
        c = (ctypes.c_int64 * 3)()
        _lib.call('mmvid_graph_stats', c)
        return list(c)

    _lib.call('mmvid_set_option', b'graphs', 0)
    before = stats()
    with pytest.raises(_lib.MMVIDError, match=r'op 1 .*STRICT with SPLIT'):
        _lib.call('mmvid_vqgan_run', arr, 2, ops._p(arena), ops._stream())
    torch.cuda.synchronize()
    assert bool((arena == 0xA5).all()) and stats() == before
