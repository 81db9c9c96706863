"""CPU checks of the weight average (GCPTrainStep(ema_decay=...), train.py --ema_decay): the warm-up sequence, the argument validation of
the two exports (before any HIP call: there is no GPU here), the checkpoint's "ema" entry with a stand-in model, and the flags of the
three entry points."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import ema_refs as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from video_gcp_amd import runtime
    if not os.path.exists(runtime.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return runtime.load_library()


# ----------------------------------------------------------------------------------------------------------------------
# the warm-up
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.999, 0.9999])
def test_warmup_values(decay):
    """min(decay, (1 + t) / (10 + t)): 0.1, 2 / 11, 10 / 19, then the cap -- (1 + t) / (10 + t) passes 0.999 at t = 8990 and 0.9999 at
    t = 89990, so t = 10^3 is still on the ramp for both and t = 10^6 is capped for both"""
    want = {0: 0.1, 1: 2.0 / 11.0, 9: 10.0 / 19.0, 10 ** 3: 1001.0 / 1010.0, 10 ** 6: decay}
    for t, w in want.items():
        assert E.warmup_decay(decay, t) == w, (decay, t)
        assert E.warmup_decay(decay, t, warmup=False) == decay
    assert 1001.0 / 1010.0 < 0.999 < 0.9999 < (1.0 + 10 ** 6) / (10.0 + 10 ** 6)
    seq = [E.warmup_decay(decay, t) for t in range(0, 200000, 997)]
    assert all(a <= b for a, b in zip(seq[:-1], seq[1:])) and seq[-1] == decay


def test_trainer_uses_the_same_sequence():
    """GCPTrainStep.ema_decay_at needs only the two settings: called on a bare object"""
    from video_gcp_amd.training import GCPTrainStep
    from types import SimpleNamespace
    for decay in (0.999, 0.9999):
        for warm in (True, False):
            s = SimpleNamespace(ema_decay=decay, ema_warmup=warm)
            for t in (0, 1, 9, 10 ** 3, 10 ** 6):
                assert GCPTrainStep.ema_decay_at(s, t) == E.warmup_decay(decay, t, warm)


def test_omd_is_exact_from_one_half():
    for decay in (0.5, 0.9, 0.999, 0.9999):
        assert float(E.omd32(decay)) == 1.0 - float(np.float32(decay))          # Sterbenz: no rounding in the float32 subtraction


# ----------------------------------------------------------------------------------------------------------------------
# the exports
# ----------------------------------------------------------------------------------------------------------------------
def test_invalid_args_are_rejected_without_a_gpu(lib):
    """argument validation happens before any HIP call"""
    a = np.full(16, 3.0, dtype=np.float32)
    b = np.full(16, 5.0, dtype=np.float32)
    pa, pb = a.ctypes.data, b.ctypes.data
    for decay, word in ((0.0, b"decay"), (1.0, b"decay"), (-0.5, b"decay"), (1.5, b"decay"), (float("nan"), b"decay"),
                        (float("inf"), b"decay")):
        assert lib.gcpx_ema_update(pa, pb, 4, decay, None, 0, None) == -1, decay
        msg = lib.gcpx_last_error()
        assert b"gcpx_ema_update" in msg and word in msg, (decay, msg)
    for args, word in (((pa, pb, -1, 0.9, None, 0, None), b"n >= 0"), ((None, pb, 4, 0.9, None, 0, None), b"null"),
                       ((pa, None, 4, 0.9, None, 0, None), b"null"), ((pa, pb, 4, 0.9, None, -1, None), b"max_blocks"),
                       ((pa + 2, pb, 2, 0.9, None, 0, None), b"aligned")):
        assert lib.gcpx_ema_update(*args) == -1, args
        msg = lib.gcpx_last_error()
        assert b"gcpx_ema_update" in msg and word in msg, (args, msg)
    assert lib.gcpx_ema_update(None, None, 0, 0.9, None, 0, None) == 0            # n = 0: nothing is launched
    for args, word in (((pa, pb, -1, 0, None), b"n >= 0"), ((None, pb, 4, 0, None), b"null"), ((pa, None, 4, 0, None), b"null"),
                       ((pa, pb, 4, -1, None), b"max_blocks"), ((pa, pb + 1, 2, 0, None), b"aligned")):
        assert lib.gcpx_swap_f32(*args) == -1, args
        msg = lib.gcpx_last_error()
        assert b"gcpx_swap_f32" in msg and word in msg, (args, msg)
    assert lib.gcpx_swap_f32(None, None, 0, 0, None) == 0
    assert (a == 3.0).all() and (b == 5.0).all()


# ----------------------------------------------------------------------------------------------------------------------
# checkpoints
# ----------------------------------------------------------------------------------------------------------------------
KEYS = ("encoder.net.input.conv.weight", "cost_mdl.cost_pred.head.linear.bias")


class _M:
    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.sd = {KEYS[0]: torch.randn(4, 3, generator=g), KEYS[1]: torch.randn(1, generator=g)}

    def state_dict(self):
        return dict(self.sd)

    def load_state_dict(self, sd, strict=True):
        for k, v in sd.items():
            if k in self.sd:
                self.sd[k] = v.clone()
            elif strict:
                raise KeyError(k)


def _ema_state(seed):
    return {"decay": 0.999, "warmup": True, "updates": 7, "state_dict": _M(seed).state_dict()}


def test_checkpoint_round_trip(tmp_path):
    from video_gcp_amd import checkpoint as ck
    a, avg = _M(1), _ema_state(2)
    plain = ck.save_checkpoint(a, str(tmp_path / "plain"), 0, global_step=5)
    with_ema = ck.save_checkpoint(a, str(tmp_path / "ema"), 0, global_step=5, ema_state=avg)
    assert set(torch.load(plain)) == {"epoch", "global_step", "state_dict", "optimizer"}              # no key when none is given
    assert set(torch.load(with_ema)) == {"epoch", "global_step", "state_dict", "optimizer", "ema"}
    assert ck.read_ema_state(plain) is None
    got = ck.read_ema_state(with_ema)
    assert (got["decay"], got["warmup"], got["updates"]) == (0.999, True, 7)
    assert all(torch.equal(got["state_dict"][k], avg["state_dict"][k]) for k in KEYS)
    # the default load does not see the entry
    b = _M(3)
    ret = ck.load_weights(with_ema, b)
    assert ret == (5, 0, None) and len(ret) == 3
    assert all(torch.equal(b.sd[k], a.sd[k]) for k in KEYS)
    # use_ema: the other dict, the same return value
    c = _M(3)
    assert ck.load_weights(with_ema, c, use_ema=True) == (5, 0, None)
    assert all(torch.equal(c.sd[k], avg["state_dict"][k]) for k in KEYS)
    assert not torch.equal(c.sd[KEYS[0]], a.sd[KEYS[0]])
    # ... under a sub-module filter: only that prefix, from the average
    d = _M(3)
    before = d.sd[KEYS[0]].clone()
    ck.load_weights(with_ema, d, submodule_name="cost_mdl", use_ema=True)
    assert torch.equal(d.sd[KEYS[1]], avg["state_dict"][KEYS[1]]) and torch.equal(d.sd[KEYS[0]], before)
    with pytest.raises(ValueError):
        ck.load_weights(with_ema, _M(3), submodule_name="inv_mdl", use_ema=True)
    # strict applies to the average's keys
    raw = torch.load(with_ema)
    del raw["ema"]["state_dict"][KEYS[1]]
    torch.save(raw, with_ema)
    with pytest.raises(KeyError):
        ck.load_weights(with_ema, _M(3), use_ema=True)
    ck.load_weights(with_ema, _M(3), use_ema=True, strict=False)
    ck.load_weights(with_ema, _M(3))                                  # the weights themselves are whole
    # a file without an average
    with pytest.raises(ValueError) as err:
        ck.load_weights(plain, _M(3), use_ema=True)
    assert plain in str(err.value)
    with pytest.raises(ValueError):
        ck.load_weights(plain, _M(3), submodule_name="cost_mdl", use_ema=True)


# ----------------------------------------------------------------------------------------------------------------------
# entry points
# ----------------------------------------------------------------------------------------------------------------------
def test_train_flags():
    from video_gcp_amd.train import ema_kwargs, get_cmd_args
    from video_gcp_amd.training import GCPTrainStep
    from video_gcp_amd.training_sequential import SequentialTrainStep
    a = get_cmd_args([])
    assert (a.ema_decay, a.ema_warmup, a.eval_ema) == (0.0, 1, 1)
    assert ema_kwargs(a) == {} and ema_kwargs(get_cmd_args(["--ema_decay", "0"])) == {}          # the trainer as it always was
    a = get_cmd_args(["--ema_decay", "0.999", "--ema_warmup", "0", "--eval_ema", "0"])
    assert (a.ema_decay, a.ema_warmup, a.eval_ema) == (0.999, 0, 0)
    assert ema_kwargs(a) == dict(ema_decay=0.999, ema_warmup=False)
    assert ema_kwargs(get_cmd_args(["--ema_decay", "0.9"])) == dict(ema_decay=0.9, ema_warmup=True)
    for bad in ("1", "-0.1", "1.5"):
        with pytest.raises(SystemExit):
            get_cmd_args(["--ema_decay", bad])
    # a trainer built without the argument holds no tensor: the defaults are None, on the class and in the signature
    sig = inspect.signature(GCPTrainStep.__init__).parameters
    assert sig["ema_decay"].default is None and sig["ema_warmup"].default is True
    assert GCPTrainStep.ema is None and SequentialTrainStep.ema is None and GCPTrainStep.ema_updates == 0


def test_plan_and_control_flags():
    from video_gcp_amd import control as CT
    from video_gcp_amd import plan as PL
    assert PL.get_args([]).use_ema == 0 and PL.get_args(["--use_ema", "1", "--weights", "w.pth"]).use_ema == 1
    base = ["--experiment", "conf.py", "--out", "out"]
    assert CT.get_args(base).use_ema == 0 and CT.get_args(base + ["--use_ema", "1"]).use_ema == 1
    from video_gcp_amd.conf_loader import build_policy
    assert inspect.signature(build_policy).parameters["use_ema"].default is False
