"""The guarded optimizer step (global-norm clip, non-finite skip, weight EMA) without a GPU: the new C-ABI symbols are
declared, bound and exported and refuse bad arguments before any launch; MuAdamW validates its new constructor arguments;
the state dict carries the EMA and the skipped count.  Nothing is launched here."""
import ctypes as C
import os
import re

import pytest
import torch

from video_diffusion_speedrun_amd import _lib, checkpoint, optim

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vds_grad_sumsq_workspace_floats", "vds_grad_sumsq_multi", "vds_optim_guard_finalize", "vds_adamw_guarded_multi",
       "vds_adamw_guarded_multi_dev", "vds_all_reduce_f32_sum")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_new_symbols_are_declared_bound_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vds.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vds_[a-z0-9_]+)\s*\(", src))
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
    assert "typedef struct vds_optim_guard" in src and C.sizeof(_lib.OptimGuard) == 16
    assert C.sizeof(_lib.AdamWTensor) == 56  # the EMA pointers did NOT go into the descriptor
    assert lib.vds_grad_sumsq_workspace_floats.restype is C.c_int64


def test_bad_arguments_are_refused_before_any_launch(lib):
    one = C.c_void_p(16)  # a non-null dummy: every call below must fail on ANOTHER argument before touching it
    assert lib.vds_grad_sumsq_workspace_floats(0) == 1 and lib.vds_grad_sumsq_workspace_floats(10301) == 10301
    # null tables / workspace / output
    assert lib.vds_grad_sumsq_multi(None, None, None, 1, 1024, None, None, 1.0, 1, None, None) == -1
    assert lib.vds_grad_sumsq_multi(one, one, one, 1, 1024, None, one, 1.0, 1, None, None) == -1
    assert lib.vds_grad_sumsq_multi(one, one, one, 1, 1024, one, None, 1.0, 1, None, None) == -1
    assert lib.vds_grad_sumsq_multi(one, one, one, 1, 2, one, one, 1.0, 1, None, None) == -1      # chunk_elems < 4
    assert lib.vds_grad_sumsq_multi(one, one, one, -1, 1024, one, one, 1.0, 1, None, None) == -1
    assert lib.vds_optim_guard_finalize(None, 1.0, 1.0, 1, one, None) == -1
    assert lib.vds_optim_guard_finalize(one, 1.0, 1.0, 1, None, None) == -1                        # null record
    ok = (0.95, 0.99, 1e-8)
    assert lib.vds_adamw_guarded_multi(None, None, None, 1, 1024, *ok, 1, 1.0, 1.0, one, None, 0.0, None) == -1
    assert lib.vds_adamw_guarded_multi(one, one, one, 1, 1024, *ok, 1, 1.0, 1.0, None, None, 0.0, None) == -1  # null record
    assert lib.vds_adamw_guarded_multi(one, one, one, 1, 2, *ok, 1, 1.0, 1.0, one, None, 0.0, None) == -1      # chunk_elems
    assert lib.vds_adamw_guarded_multi(one, one, one, 1, 1024, *ok, 0, 1.0, 1.0, one, None, 0.0, None) == -1   # step < 1
    assert lib.vds_adamw_guarded_multi(one, one, one, 1, 1024, *ok, 1, 1.0, 1.0, one, one, 1.0, None) == -1    # decay = 1
    assert lib.vds_adamw_guarded_multi_dev(None, None, None, 1, 1024, *ok, one, 1.0, one, None, None) == -1
    assert lib.vds_adamw_guarded_multi_dev(one, one, one, 1, 1024, *ok, None, 1.0, one, None, None) == -1      # null scalars
    assert lib.vds_adamw_guarded_multi_dev(one, one, one, 1, 1024, *ok, one, 1.0, None, None, None) == -1      # null record
    assert lib.vds_adamw_guarded_multi_dev(one, one, one, 1, 3, *ok, one, 1.0, one, None, None) == -1
    # an empty work list is fine and launches nothing
    assert lib.vds_adamw_guarded_multi(one, one, one, 0, 1024, *ok, 1, 1.0, 1.0, one, None, 0.0, None) == 0
    assert lib.vds_all_reduce_f32_sum(None, 1, None) < 0  # no communicator in this process (and a null buffer)


def test_constructor_validation():
    p = [torch.nn.Parameter(torch.zeros(4))]
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            optim.MuAdamW(p, max_grad_norm=bad)
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            optim.MuAdamW(p, ema_decay=bad)
    o = optim.MuAdamW(p, max_grad_norm=float("inf"), ema_decay=0.0, skip_nonfinite=True)
    assert o.guarded and o.max_grad_norm == float("inf") and o.ema_decay == 0.0 and o.skipped_steps() == 0
    with pytest.raises(ValueError):
        o.ema_decay = 1.0
    o.ema_decay = 0.999
    assert o.ema_decay == 0.999
    plain = optim.MuAdamW(p)
    assert not plain.guarded and plain.grad_norm is None and "vds_skipped" not in plain.state_dict()


def test_state_dict_round_trip_carries_ema_and_skipped_count(tmp_path):
    ps = [torch.nn.Parameter(torch.arange(6.0).view(2, 3)), torch.nn.Parameter(torch.ones(5))]
    o = optim.MuAdamW(ps, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
    for i, p in enumerate(ps):  # the state a few steps leave behind
        o.state[p] = {"exp_avg": torch.full((p.numel(),), 0.5 + i), "exp_avg_sq": torch.full((p.numel(),), 0.25),
                      "ema": p.detach().clone() * 3 + i}
    o._step, o._skipped_seed = 7, 2
    sd = o.state_dict()
    assert sd["vds_step"] == 7 and sd["vds_skipped"] == 2
    torch.save(sd, tmp_path / "o.pt")
    sd = torch.load(tmp_path / "o.pt", weights_only=True)  # what checkpoint.load_checkpoint does
    ps2 = [torch.nn.Parameter(torch.zeros(2, 3)), torch.nn.Parameter(torch.zeros(5))]
    o2 = optim.MuAdamW(ps2, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.9)
    o2.load_state_dict(sd)
    assert o2._step == 7 and o2.skipped_steps() == 2
    for p, q in zip(ps, ps2):
        assert torch.equal(o2.state[q]["ema"], o.state[p]["ema"]) and o2.state[q]["ema"].shape == q.shape
        assert torch.equal(o2.state[q]["exp_avg"], o.state[p]["exp_avg"])
    # swapping twice restores every bit (plumbing: torch copies, works on any device)
    before = [(p.detach().clone(), o.state[p]["ema"].clone()) for p in ps]
    o.swap_ema()
    assert all(torch.equal(p.detach(), e0) and torch.equal(o.state[p]["ema"], p0) for p, (p0, e0) in zip(ps, before))
    o.swap_ema()
    assert all(torch.equal(p.detach(), p0) and torch.equal(o.state[p]["ema"], e0) for p, (p0, e0) in zip(ps, before))
    with pytest.raises(FileNotFoundError):
        checkpoint.read_model_state(str(tmp_path), ema=True)
