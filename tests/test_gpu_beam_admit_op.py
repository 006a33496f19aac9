"""Operator-level test of beam_admit_kernel (csrc/decode_admit.hip) through its C ABI entry itts_beam_admit: the beam state of a
fresh generation for n of 5 batch items, on caller buffers filled with sentinels.  Every byte of every buffer - a guard block
behind each included - is compared with a numpy restatement of what the kernel has to write: the admitted items' running scores
(0; beam_search: 0 for the first beam and -1e9 behind it), BOTH halves of their ancestry rows (row item * nb + q filled with q, the
half base at items * nb * Smax), hyp_order = -1, hyp_n = 0, hyp_worst = 1e9, hyp_counter = 0, done = 0 and - draws given - their
column of uniforms [max_gen][items][2 * nb].  Everything else must keep its sentinel: the other items, the draws when no source
is given, the guards.  The sentinels differ from element to element, so a write to a wrong place cannot land on an equal value."""
import ctypes as C

import numpy as np
import pytest
import torch

from itts_hip import lib as L
from test_gpu_decode_gemv import stream, sync

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ITEMS, GUARD = 5, 64
SHAPES = [(256, 7), (256, 33), (512, 7), (512, 33)]  # Smax, max_gen


@pytest.mark.parametrize("draws", [True, False])
@pytest.mark.parametrize("do_sample", [1, 0])
@pytest.mark.parametrize("admitted", [[0], [4], [1, 3], [0, 1, 2, 3, 4], [3, 0]])
@pytest.mark.parametrize("nb", [2, 3, 10])
def test_beam_admit_every_byte(nb, admitted, do_sample, draws):
    lib = L.load()
    n, rows, nd = len(admitted), ITEMS * nb, 2 * nb
    for Smax, mg in SHAPES:
        rng = np.random.default_rng(nb * 100000 + Smax * 100 + mg + 7 * n)
        sizes = dict(beam_scores=rows, anc=2 * rows * Smax, hyp_order=ITEMS * (nb + 1), hyp_n=ITEMS, hyp_worst=ITEMS, hyp_counter=ITEMS,
                     beam_done=ITEMS, uniforms=mg * ITEMS * nd)
        host = {}
        for k, sz in sizes.items():
            if k == "anc":
                host[k] = rng.integers(11, 256, sz + GUARD).astype(np.uint8)  # (never a beam index 0 .. 10)
            elif k in ("beam_scores", "hyp_worst", "uniforms"):
                host[k] = (rng.random(sz + GUARD, dtype=np.float32) + 2.0).astype(np.float32)  # (never 0, -1e9, 1e9 or a draw in [0, 1))
            else:
                host[k] = rng.integers(100, 1 << 20, sz + GUARD).astype(np.int32)
        usrc = rng.random((n, mg, nd), dtype=np.float32)
        dev = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in host.items()}
        us = torch.from_numpy(usrc).to(DEV)
        it = np.asarray(admitted, dtype=np.int32)
        a = L.BeamAdmitArgs(**{k: v.data_ptr() for k, v in dev.items()}, uniforms_src=us.data_ptr() if draws else None,
                            items_host=it.ctypes.data, n=n, nb=nb, items=ITEMS, Smax=Smax, max_gen=mg, do_sample=do_sample)
        L.check(lib.itts_beam_admit(C.byref(a), stream()), "beam_admit", lib)
        sync()
        want = {k: v.copy() for k, v in host.items()}
        anc = want["anc"][:2 * rows * Smax].reshape(2, rows, Smax)
        u = want["uniforms"][:mg * ITEMS * nd].reshape(mg, ITEMS, nd)
        ho = want["hyp_order"][:ITEMS * (nb + 1)].reshape(ITEMS, nb + 1)
        for i, g in enumerate(admitted):
            for q in range(nb):
                want["beam_scores"][g * nb + q] = 0.0 if (do_sample or q == 0) else -1e9
                anc[:, g * nb + q, :] = q
            ho[g] = -1
            want["hyp_n"][g], want["hyp_worst"][g], want["hyp_counter"][g], want["beam_done"][g] = 0, 1e9, 0, 0
            if draws:
                u[:, g] = usrc[i]
        for k, v in want.items():
            got = dev[k].cpu().numpy()
            same = np.array_equal(got.view(np.uint8), v.view(np.uint8))
            assert same, (k, Smax, mg, np.argwhere(got != v)[:4].ravel().tolist())
        assert not np.array_equal(want["anc"], host["anc"]) and not np.array_equal(want["hyp_order"], host["hyp_order"])


def test_beam_admit_without_a_draws_table():
    """beam_search: uniforms and uniforms_src both null."""
    lib = L.load()
    nb, Smax, mg, rows = 3, 256, 7, ITEMS * 3
    dev = dict(beam_scores=torch.full((rows,), 5.0, device=DEV), anc=torch.full((2 * rows * Smax,), 77, dtype=torch.uint8, device=DEV),
               hyp_order=torch.full((ITEMS * (nb + 1),), 9, dtype=torch.int32, device=DEV), hyp_n=torch.full((ITEMS,), 9, dtype=torch.int32, device=DEV),
               hyp_worst=torch.full((ITEMS,), 5.0, device=DEV), hyp_counter=torch.full((ITEMS,), 9, dtype=torch.int32, device=DEV),
               beam_done=torch.full((ITEMS,), 1, dtype=torch.int32, device=DEV))
    it = np.asarray([2], dtype=np.int32)
    a = L.BeamAdmitArgs(**{k: v.data_ptr() for k, v in dev.items()}, uniforms=None, uniforms_src=None, items_host=it.ctypes.data, n=1, nb=nb,
                        items=ITEMS, Smax=Smax, max_gen=mg, do_sample=0)
    L.check(lib.itts_beam_admit(C.byref(a), stream()), "beam_admit", lib)
    sync()
    assert dev["beam_scores"].cpu().tolist() == [5.0] * 6 + [0.0, -1e9, -1e9] + [5.0] * 6
    anc = dev["anc"].cpu().numpy().reshape(2, rows, Smax)
    assert np.all(anc[:, 6:9] == np.arange(3, dtype=np.uint8)[None, :, None]) and np.all(anc[:, :6] == 77) and np.all(anc[:, 9:] == 77)
    assert dev["beam_done"].cpu().tolist() == [1, 1, 0, 1, 1] and dev["hyp_n"].cpu().tolist() == [9, 9, 0, 9, 9]
    assert dev["hyp_order"].cpu().tolist() == [9] * 8 + [-1] * 4 + [9] * 8
