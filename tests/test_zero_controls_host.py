"""Zero controls, the parts that need no GPU: the C ABI refuses a null model first whatever the control pointers are, the Python binding
turns None controls into NULL arguments, and the checkpointed ForwardWarp slices only the controls that exist.
Two of these hold before the feature as well -- the null-model refusal and the binding, which already mapped None to NULL: they pin
what the feature relies on and do not show that it works.  The checkpointed-slicing test here and tests/test_gpu_zero_controls.py do."""
import ctypes
import os

import pytest
import torch

from helpers import ROOT

LIB = os.path.join(ROOT, "ppr-diffphys_amd", "diffphys_amd", "lib", "libpprdiffphys_hip.so")


def test_null_model_is_refused_first_whatever_the_control_pointers():
    """All six rollout entries, with the torques / res_f arguments NULL and non-NULL (a dangling value that must never be read): the
    null model is what is refused, before any pointer is looked at."""
    lib = ctypes.CDLL(LIB)
    lib.pd_last_error.restype = ctypes.c_char_p
    err = lambda: lib.pd_last_error().decode()
    f2s = (ctypes.c_int * 2)(0, 1)
    vp, cf = ctypes.c_void_p, ctypes.c_float(5e-4)
    junk = vp(0x1000)
    for tq, rf in ((None, None), (junk, None), (None, junk), (junk, junk)):
        fwd = [junk, junk, tq, rf] + [junk] * 6     # q_init, qd_init, torques, res_f, refs, ke, kd, inv_mass, inertia, inv_inertia
        bwd = [junk, junk, tq] + [junk] * 6         # q_init, qd_init, torques, refs, ...
        loss_f = [None, None, ctypes.c_float(0.1)] + [None] * 5
        calls = [
            lambda: lib.pd_rollout_forward(None, 1, 1, cf, *fwd, 2, f2s, *([None] * 5), None),
            lambda: lib.pd_rollout_forward_traj_loss(None, 1, 1, cf, *fwd, 2, f2s, *([None] * 5), *loss_f, None),
            lambda: lib.pd_rollout_forward_traj_loss_fk(None, 1, 1, cf, *fwd, 2, f2s, *([None] * 5), *loss_f, None, None),
            lambda: lib.pd_rollout_backward(None, 1, 1, cf, *bwd, 2, f2s, *([None] * 13), None),
            lambda: lib.pd_rollout_backward_traj_loss(None, 1, 1, cf, *bwd, 2, f2s, *([None] * 17), None),
            lambda: lib.pd_rollout_backward_traj_loss_fk(None, 1, 1, cf, *bwd, 2, f2s, *([None] * 17), None, None),
        ]
        for i, call in enumerate(calls):
            assert call() != 0 and "null model" in err(), (i, err())


class _FakeTensor:
    """what hip_backend._dev asks of a tensor, with no device behind it"""
    is_cuda, dtype, device = True, torch.float32, "fake"

    def __init__(self, n, ptr):
        self._n, self._ptr = n, ptr

    def numel(self):
        return self._n

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self._ptr


class _FakeLib:
    def __init__(self):
        self.calls = []

    def pd_rollout_workspace_floats(self, h, bs, nsteps):
        return 1000 * bs * nsteps

    def __getattr__(self, name):
        if not name.startswith("pd_rollout_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return 0

        return entry


def _fake_model(monkeypatch):
    from diffphys_amd import hip_backend

    fake = _FakeLib()
    monkeypatch.setattr(hip_backend, "lib", lambda: fake)
    monkeypatch.setattr(hip_backend, "_stream", lambda: 0)
    dm = object.__new__(hip_backend.DeviceModel)
    dm.h, dm.nb, dm.nq, dm.nqd, dm._xp = 77, 13, 19, 18, None
    return dm, fake


def test_binding_passes_null_for_none_controls(monkeypatch):
    """DeviceModel.rollout_forward / rollout_forward_traj_loss / rollout_backward / rollout_backward_traj_loss with None for torques and
    res_f: positions unchanged, the library gets NULL for exactly those arguments, every other size is still checked against refs and the
    model."""
    dm, fake = _fake_model(monkeypatch)
    bs, T, F = 3, 5, 2
    nb, nq, nqd = dm.nb, dm.nq, dm.nqd
    n = iter(range(1, 100))
    ft = lambda numel: _FakeTensor(numel, 0x1000 * next(n))
    q, qd, refs = ft(bs * nq), ft(bs * nqd), ft(T * bs * nqd)
    rest = [ft(bs * nqd), ft(bs * nqd), ft(bs * nb), ft(bs * nb * 9), ft(bs * nb * 9)]
    out = dict(ws=ft(1000 * bs * T), wp_pos=ft(F * bs * nb * 7), wp_vel=ft(F * bs * nb * 6), grf=ft(F * bs * nb * 6), jaf=ft(F * bs * nb * 6))
    tq, rf = ft(T * bs * nqd), ft(T * bs * nb * 6)
    for give_t, give_r in ((False, False), (True, False), (False, True)):
        del fake.calls[:]
        a_t, a_r = (tq if give_t else None), (rf if give_r else None)
        dm.rollout_forward(bs, T, 5e-4, q, qd, a_t, a_r, refs, *rest, frame2step=[0, T], out=out)
        name, args = fake.calls[-1]
        assert name == "pd_rollout_forward" and args[:4] == (77, bs, T, 5e-4)
        assert args[4:9] == (q.data_ptr(), qd.data_ptr(), a_t and a_t.data_ptr(), a_r and a_r.data_ptr(), refs.data_ptr())
        g = {k: ft(1) for k in ("q_init", "qd_init", "torques", "res_f", "refs", "target_ke", "target_kd", "body_inv_mass", "body_inertia",
                                "body_inv_inertia")}
        dm.rollout_backward(bs, T, 5e-4, q, qd, a_t, refs, *rest, [0, T], out["ws"], ft(F * bs * nb * 7), ft(F * bs * nb * 6), out=dict(grads=g))
        name, args = fake.calls[-1]
        assert name == "pd_rollout_backward" and args[4:8] == (q.data_ptr(), qd.data_ptr(), a_t and a_t.data_ptr(), refs.data_ptr())
        assert args[18:23] == tuple(g[k].data_ptr() for k in ("q_init", "qd_init", "torques", "res_f", "refs"))  # the gradients stay independent
    # a wrong size of refs is still caught; a None refs reaches the library as NULL (which refuses it by name)
    with pytest.raises((ValueError, TypeError), match="refs"):  # (TypeError: the stand-in is no torch tensor, which the slow path says first)
        dm.rollout_forward(bs, T, 5e-4, q, qd, None, None, ft(7), *rest, frame2step=[0, T], out=out)
    dm.rollout_forward(bs, T, 5e-4, q, qd, None, None, None, *rest, frame2step=[0, T], out=out)
    assert fake.calls[-1][1][6:9] == (None, None, None)


class _RecordingModel:
    """stands in for DeviceModel under the checkpointed ForwardWarp: CPU tensors, records the controls of every launch"""
    nb, nq, nqd = 2, 9, 8

    def __init__(self):
        self.fwd, self.bwd = [], []

    def workspace_floats(self, bs, nsteps):
        return 10 * bs * nsteps

    def _alloc_grads(self, bs, nsteps, device, resumed=False, want=("torques", "res_f", "refs")):
        from diffphys_amd import hip_backend

        return {k: v.zero_() for k, v in hip_backend.alloc_grads(self.nb, self.nq, self.nqd, bs, nsteps, device, resumed=resumed, want=want).items()}

    def rollout_forward(self, bs, nsteps, dt, q_init, qd_init, torques, res_f, refs, *rest, frame2step, want_forces=True, out=None,
                        save_trajectory=True, state0=None):
        self.fwd.append((nsteps, torques, res_f, refs))
        F, N = len(frame2step), bs * self.nb
        z = lambda *s: torch.zeros(*s)
        return z(F, N, 7), z(F, N, 6), z(F, N, 6), z(F, N, 6), None

    def rollout_backward(self, bs, nsteps, dt, q_init, qd_init, torques, refs, *a, out=None, state0=None, want=()):
        self.bwd.append((nsteps, torques, refs, tuple(want)))
        for v in out["grads"].values():
            v.zero_()
        return out["grads"]


def test_checkpointed_paths_slice_only_what_exists():
    """_checkpoint_forward / _checkpoint_backward over 17 steps in segments of 5 with torques and res_f absent: every segment launch gets
    None for both and its own slice of refs; with tensors, its slices of all three."""
    from diffphys_amd import dp_model

    bs, T, K, f2s = 2, 17, 5, [0, 8, 17]
    plan = dp_model.checkpoint_plan(T, f2s, K)
    assert [(s, e) for s, e, *_ in plan[1]] == [(0, 5), (5, 10), (10, 15), (15, 17)]
    nb, nq, nqd = _RecordingModel.nb, _RecordingModel.nq, _RecordingModel.nqd
    refs, tq, rf = torch.randn(T, bs * nqd), torch.zeros(T, bs * nqd), torch.zeros(T, bs * nb, 6)
    rest = [torch.ones(bs * nqd), torch.ones(bs * nqd), torch.ones(bs * nb), torch.ones(bs * nb, 3, 3), torch.ones(bs * nb, 3, 3)]
    ap, av = torch.zeros(len(f2s), bs * nb, 7), torch.zeros(len(f2s), bs * nb, 6)
    for a_t, a_r in ((None, None), (tq, None), (None, rf), (tq, rf)):
        dm = _RecordingModel()
        inp = [torch.zeros(bs * nq), torch.zeros(bs * nqd), a_t, a_r, refs] + rest
        pos, vel, grf, jaf, states = dp_model._checkpoint_forward(dm, bs, T, 5e-4, inp, f2s, K)
        assert len(dm.fwd) == 1 and dm.fwd[0][1] is a_t and dm.fwd[0][2] is a_r and states.shape == (3, bs * nb, 13)
        g = dp_model._checkpoint_backward(dm, bs, T, 5e-4, inp, f2s, K, states, ap, av, want=("refs",))
        assert set(g) >= {"q_init", "refs", "target_ke"} and "torques" not in g and "res_f" not in g
        segs = dm.fwd[1:]
        assert [s[0] for s in segs] == [2, 5, 5, 5] and [b[0] for b in dm.bwd] == [2, 5, 5, 5]
        for (n, s_t, s_r, s_refs), (_, b_t, b_refs, want) in zip(segs, dm.bwd):
            assert (s_t is None) == (a_t is None) and (s_r is None) == (a_r is None) and (b_t is None) == (a_t is None)
            assert s_refs.shape[0] == n and b_refs.shape[0] == n and want == ("refs",)
            assert s_t is None or s_t.shape[0] == n
            assert s_r is None or s_r.shape[0] == n
        assert torch.equal(torch.cat([s[3] for s in reversed(segs)]), refs)
