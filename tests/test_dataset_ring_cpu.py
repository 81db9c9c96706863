"""The slot ring of the loaders (dataset.RingLoader.__iter__) on the host: a stub loader whose three device hooks (_submit, _upload,
_assemble) only record their calls is driven for fewer batches than slots, as many, and more, once with fills that have finished when
the ring looks and once with fills that finish only when the ring waits for them.  No GPU, no thread, no waiting."""
import os
import sys
import types
from concurrent.futures import Future

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_gcp_amd  # noqa: E402,F401
from video_gcp_amd import dataset as DS  # noqa: E402


class _HeldFill(Future):
    """a fill that is not done until somebody waits for it"""

    def result(self, timeout=None):
        if not self.done():
            self.set_result(None)
        return super().result(timeout)


class _Items:
    phase, T, img_sz = "val", 4, 8

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class _StubLoader(DS.RingLoader):
    """batch k is the one item k (batch size 1, no shuffle): the hooks log (what, slot, k)"""

    def __init__(self, n_batches, n_slots, instant):
        model = types.SimpleNamespace(_hp=types.SimpleNamespace(max_seq_len=_Items.T, img_sz=_Items.img_sz, batch_size=1), device="cpu")
        super().__init__(_Items(n_batches), model, 1, 1, 0, 0, 1, n_slots, False, 1)
        self.instant, self.log, self.pinned, self.on_device, self.fills = instant, [], {}, {}, {}

    def _submit(self, slot, batch):
        k = batch[0][0]
        self.log.append(("submit", slot, k))
        self.pinned[slot] = k
        f = Future() if self.instant else _HeldFill()
        if self.instant:
            f.set_result(None)
        self.fills[k] = f
        return [f]

    def _upload(self, slot):
        k = self.pinned[slot]
        assert self.fills[k].done(), f"batch {k} uploaded before its fill was waited for"
        self.log.append(("upload", slot, k))
        self.on_device[slot] = k

    def _assemble(self, slot):
        k = self.on_device[slot]
        self.log.append(("assemble", slot, k))
        return k


@pytest.mark.parametrize("instant", [True, False], ids=["instant_fills", "held_fills"])
@pytest.mark.parametrize("n_slots", [2, 3])
@pytest.mark.parametrize("n_batches", [1, 2, 3, 5])
def test_ring_order(n_batches, n_slots, instant):
    loader = _StubLoader(n_batches, n_slots, instant)
    assert len(loader) == n_batches and [b[0][0] for b in loader.schedule()] == list(range(n_batches))
    yielded = []
    for k in loader:
        loader.log.append(("yield", k % n_slots, k))
        yielded.append(k)
    assert yielded == list(range(n_batches))                                  # schedule order
    log = loader.log
    at = lambda what, k: log.index((what, k % n_slots, k))                    # raises when the call is missing or on another slot
    for k in range(n_batches):
        assert sum(1 for e in log if e[0] == "upload" and e[2] == k) == 1     # uploaded exactly once ...
        assert sum(1 for e in log if e[0] == "submit" and e[2] == k) == 1
        assert at("submit", k) < at("upload", k) < at("assemble", k) < at("yield", k)         # ... and before its assembly
        if k + n_slots < n_batches:                                           # the slot is resubmitted only after batch k was assembled
            assert at("assemble", k) < at("submit", k + n_slots)
        if instant and k + 1 < n_batches:                                     # the overlap: the next upload is issued under this step
            assert at("upload", k + 1) < at("yield", k)
    assert len(log) == 4 * n_batches
