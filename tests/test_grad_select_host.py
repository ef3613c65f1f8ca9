"""Selective adjoint, the parts that need no GPU: the binding's ``want`` handling, the map from an autograd ctx's ``needs_input_grad`` to
``want`` for each Function's argument order, and the library's argument check order."""
import ctypes
import inspect

import pytest
import torch


def test_want_handling_of_the_binding():
    from diffphys_amd import hip_backend

    assert hip_backend.GRAD_NAMES == ("torques", "res_f", "refs")
    assert hip_backend.grad_want(hip_backend.GRAD_NAMES) == hip_backend.GRAD_NAMES
    assert hip_backend.grad_want(()) == () and hip_backend.grad_want([]) == ()
    assert hip_backend.grad_want(["refs", "torques"]) == ("torques", "refs")   # GRAD_NAMES order, whatever the caller's
    assert hip_backend.grad_want("res_f") == ("res_f",)
    for bad in (("torque",), ("q_init",), ("torques", "target_ke"), "t"):
        with pytest.raises(ValueError, match="unknown per-step gradient"):
            hip_backend.grad_want(bad)
    # the default of both entry points is all three: an existing caller sees the dictionary it always got
    for fn in (hip_backend.DeviceModel.rollout_backward, hip_backend.DeviceModel.rollout_backward_traj_loss, hip_backend.DeviceModel._alloc_grads):
        assert inspect.signature(fn).parameters["want"].default == hip_backend.GRAD_NAMES


def test_unwanted_gradients_are_neither_allocated_nor_returned():
    from diffphys_amd import hip_backend

    nb, nq, nqd, bs, T = 13, 19, 18, 3, 4
    always = {"q_init", "qd_init", "target_ke", "target_kd", "body_inv_mass", "body_inertia", "body_inv_inertia"}
    g = hip_backend.alloc_grads(nb, nq, nqd, bs, T, "cpu")
    assert set(g) == always | {"torques", "res_f", "refs"}
    assert g["torques"].shape == (T, bs * nqd) and g["res_f"].shape == (T, bs * nb, 6) and g["refs"].shape == (T, bs * nqd)
    assert set(hip_backend.alloc_grads(nb, nq, nqd, bs, T, "cpu", want=())) == always
    g = hip_backend.alloc_grads(nb, nq, nqd, bs, T, "cpu", want=("res_f",))
    assert set(g) == always | {"res_f"} and g["res_f"].shape == (T, bs * nb, 6)
    g = hip_backend.alloc_grads(nb, nq, nqd, bs, T, "cpu", resumed=True, want=("torques",))
    assert set(g) == (always - {"q_init", "qd_init"}) | {"state0", "torques"} and g["state0"].shape == (bs * nb, 13)
    with pytest.raises(ValueError):
        hip_backend.alloc_grads(nb, nq, nqd, bs, T, "cpu", want=("ref",))
    # caller-provided buffers (out=): an unwanted name is dropped from what comes back, a wanted one must be there
    full = hip_backend.alloc_grads(nb, nq, nqd, bs, T, "cpu")
    assert hip_backend._select_grads(full, hip_backend.GRAD_NAMES) is full
    sel = hip_backend._select_grads(full, ("refs",))
    assert set(sel) == always | {"refs"} and sel["refs"] is full["refs"]
    with pytest.raises(KeyError, match="torques"):
        hip_backend._select_grads(sel, ("torques", "refs"))


def test_needs_input_grad_maps_to_want_for_every_function():
    """torques, res_f and refs are inputs 2, 3 and 4 of all four Functions (ctx aside): grads_wanted reads those positions."""
    from diffphys_amd import dp_model

    for cls in (dp_model.ForwardWarp, dp_model.ForwardWarpState, dp_model.ForwardWarpTrajLoss, dp_model.ForwardWarpTrajLossFK):
        params = list(inspect.signature(cls.forward).parameters)[1:]   # without ctx
        pos = {n: params.index(n) for n in ("torques", "res_f", "refs")}
        assert pos == dict(torques=2, res_f=3, refs=4), (cls.__name__, pos)
        n = len(params)
        for mask in range(8):
            needs = [False] * n
            chosen = tuple(name for j, name in enumerate(("torques", "res_f", "refs")) if mask >> j & 1)
            for name in chosen:
                needs[pos[name]] = True
            assert dp_model.grads_wanted(tuple(needs)) == chosen, (cls.__name__, mask)
            # what the OTHER inputs need does not matter
            others = [True] * n
            for name in ("torques", "res_f", "refs"):
                others[pos[name]] = needs[pos[name]]
            assert dp_model.grads_wanted(tuple(others)) == chosen


def test_functions_return_none_for_what_was_not_asked_with_a_fake_backend():
    """ForwardWarp.backward hands autograd None for an unwanted per-step gradient and passes ``want`` on (no GPU: a fake DeviceModel)."""
    from diffphys_amd import dp_model, hip_backend

    nb, nq, nqd, bs, T = 2, 8, 7, 2, 3
    seen = []

    class FakeDM:
        pass

    dm = FakeDM()
    dm.nb, dm.nq, dm.nqd = nb, nq, nqd

    def rollout_forward(bs_, nsteps, dt, *inp, frame2step, **kw):
        F = len(frame2step)
        z = lambda *s: torch.zeros(*s)
        return z(F, bs * nb, 7) + inp[0].sum() * 0, z(F, bs * nb, 6), z(F, bs * nb, 6), z(F, bs * nb, 6), z(4)

    def rollout_backward(bs_, nsteps, dt, *args, want=hip_backend.GRAD_NAMES, **kw):
        seen.append(tuple(want))
        return {k: torch.ones_like(v) for k, v in hip_backend.alloc_grads(nb, nq, nqd, bs, T, "cpu", want=want).items()}

    dm.rollout_forward, dm.rollout_backward = rollout_forward, rollout_backward

    class Env:
        _handle = dm

    class Host:
        pass

    h = Host()
    h.env, h.num_envs, h.steps_idx, h.frame2step, h.dt = Env(), bs, range(T), [0, T], 5e-4
    shapes = dict(q_init=(bs * nq,), qd_init=(bs * nqd,), torques=(T, bs * nqd), res_f=(T, bs * nb, 6), refs=(T, bs * nqd), target_ke=(bs * nqd,),
                  target_kd=(bs * nqd,), body_mass=(bs * nb,), body_inv_mass=(bs * nb,), body_inertia=(bs * nb, 3, 3), body_inv_inertia=(bs * nb, 3, 3))
    for needs in (("refs", "target_ke"), ("q_init",), tuple(shapes)):
        t = {k: torch.zeros(*s, requires_grad=k in needs) for k, s in shapes.items()}
        pos, vel = dp_model.ForwardWarp.apply(*t.values(), h)
        (pos.sum() + vel.sum()).backward()
        assert seen[-1] == tuple(k for k in ("torques", "res_f", "refs") if k in needs)
        for k in shapes:
            assert (t[k].grad is not None) == (k in needs), (needs, k)


def test_library_answers_null_model_before_it_looks_at_any_pointer():
    """Loaded without a GPU: the three backward entries refuse a null model first, whatever the gradient pointers are."""
    from diffphys_amd import hip_backend

    lib = hip_backend.lib()
    err = lambda: lib.pd_last_error().decode()
    f2s = (ctypes.c_int * 2)(0, 1)
    junk = ctypes.c_void_p(64)   # never dereferenced: the model is checked first
    for g3 in ((None, None, None), (junk, None, junk), (junk, junk, junk)):
        grads = [junk, junk, *g3] + [junk] * 5
        assert lib.pd_rollout_backward(None, 1, 1, ctypes.c_float(5e-4), *([None] * 9), 2, f2s, *([None] * 3), *grads, None) != 0
        assert "null model" in err()
        assert lib.pd_rollout_backward_traj_loss(None, 1, 1, ctypes.c_float(5e-4), *([None] * 9), 2, f2s, *([None] * 7), *grads, None) != 0
        assert "null model" in err()
        assert lib.pd_rollout_backward_traj_loss_fk(None, 1, 1, ctypes.c_float(5e-4), *([None] * 9), 2, f2s, *([None] * 7), *grads, None, None) != 0
        assert "null model" in err()
