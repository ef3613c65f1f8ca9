"""Forward-only rollouts: pd_rollout_forward / pd_rollout_forward_traj_loss(_fk) with workspace_dev == NULL (k_rollout_fwd SAVE = false).
Such a launch stores no trajectory, no hit log and no loss seeds, and must give every output it does write -- frame poses, twists,
ground / joint wrenches, loss table, reduced loss, scale, FK rows -- BIT FOR BIT as the saving launch does: the kernels differ only by
the dropped stores.  ForwardWarp / ForwardWarpTrajLoss(FK) take that path when no input needs a gradient (torch.no_grad())."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from gpu_harness import BWD, FWD, dev, dev_inputs, warp_host  # noqa: F401

pytestmark = pytest.mark.gpu



def _template(key, tmp_path):
    from diffphys_amd import robots

    if key in ("laikago", "human", "quad"):
        return robots.load_template(key), key
    if key == "toy":   # free + revolute + compound + fixed joints: the generic instantiation
        from helpers import toy_template

        return toy_template(tmp_path), None
    from test_gpu_large_contact_sets import replicated, toes_template

    if key == "laikago_toes":   # fixed toe joints, 11 018 candidates: tables in global memory, generic split kernel
        return toes_template(), "laikago"
    if key == "laikago12k":     # revolute-only with tables in global memory: both kernel families
        return replicated("laikago", 12000), "laikago"
    raise KeyError(key)


def _inputs(tpl, robot, bs, T, seed=0):
    from diffphys_amd import synth
    from helpers import toy_inputs

    if robot is None:
        inp = toy_inputs(tpl, bs, T, list(range(0, T + 1, 20)), seed=seed)
    else:
        inp = synth.make_inputs(tpl, robot, bs=bs, nsteps=T, seed=seed, steps_per_frame=20, penetration=0.003)
    return inp


def _variant(dm, info, family):
    """what pd_last_launch_info says ran: 'quad' / 'quad-2role' (quad-lane family: one env per wave pair, with / without the cull wave),
    'cullw+runsum' / 'cullw' (body, contact and cull wave per env group; four groups per workgroup = RUNSUM), 'split' (body + contact
    wave), 'unsplit' (one wave per env group)"""
    waves, envs = info["threads_per_wg"] // 64, info["envs_per_wg"]
    if family == 2:
        assert envs <= 4, info
        return "quad" if waves == 3 * envs else ("quad-2role" if waves == 2 * envs else "?")
    groups = envs // (64 // dm.segment_width())
    if waves == 3 * groups:
        return "cullw+runsum" if groups == 4 else "cullw"
    return {2 * groups: "split", groups: "unsplit"}.get(waves, "?")


# (model, bs, kernel family, segment widths, the variant pd_last_launch_info must report)
CASES = [
    ("laikago", 512, 2, (64,), ("quad",)),              # quad-lane family with the cull wave
    ("laikago", 4096, 0, (16, 32, 64), ("cullw+runsum",)),
    ("laikago", 256, 1, (16, 32, 64), ("cullw",)),     # a batch below full workgroups: the cull wave without RUNSUM
    ("human", 1024, 0, (32, 64), ("split",)),           # compound-only, latency regime: split
    ("quad", 8192, 0, (32, 64), ("unsplit",)),          # compound-only above 4 x CUs env groups: unsplit
    ("toy", 512, 0, (16, 32, 64), ("split",)),          # generic joint mix
    ("laikago_toes", 256, 0, (64,), ("split",)),        # tables in global memory (GT), generic
    # GT, revolute-only: lane per body and quad-lane (with the cull wave where its list fits the per-env LDS, else two roles)
    ("laikago12k", 256, 1, (None,), ("cullw", "split")),
    ("laikago12k", 37, 2, (64,), ("quad", "quad-2role")),
]


def _ids(c):
    return "%s-%d-f%d" % c[:3]


def _run_pair(dm, inp, dev, loss):
    """the same launch with and without a workspace -> (saving, forward-only) dicts of every output, plus the launch infos"""
    bs = inp["q_init"].size // dm.nq
    T, f2s = inp["nsteps"], list(inp["frame2step"])
    t = dev_inputs(inp, dev)
    res = []
    for save in (True, False):
        if not loss:
            pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s, save_trajectory=save)
            o = dict(wp_pos=pos, wp_vel=vel, grf=grf, jaf=jaf)
        else:
            F = len(f2s)
            rng = np.random.RandomState(3)
            tgt = torch.from_numpy((rng.randn(bs, F, dm.nb, 7) * 0.05).astype(np.float32)).to(dev)
            tgt[..., 3:] = torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev)
            outseq = torch.zeros(bs, F, dtype=torch.bool, device=dev)
            outseq[1, 0] = True
            jq = t["q_init"].reshape(1, bs, dm.nq).repeat(F, 1, 1).contiguous()
            jqd = torch.from_numpy((rng.randn(F, bs, dm.nqd) * 0.1).astype(np.float32)).to(dev)
            pos, vel, grf, jaf, ws, tl = dm.rollout_forward_traj_loss(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s, target_pos=tgt,
                                                                      outseq=outseq, fk=(jq, jqd), save_trajectory=save)
            o = dict(wp_pos=pos, wp_vel=vel, grf=grf, jaf=jaf, reduced=tl["reduced"], table=tl["table"], scale=tl["scale"],
                     fk_body_q=tl["fk_body_q"], fk_body_qd=tl["fk_body_qd"])
            if not save:
                assert tl["seed_pos"] is None and tl["seed_gt"] is None
        assert (ws is None) == (not save)
        torch.cuda.synchronize()
        res.append(({k: v.clone() for k, v in o.items()}, dm.last_launch_info(0)))
    return res


@pytest.mark.parametrize("policy", ["stable", "literal"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_only_is_bit_identical_in_every_variant(dev, tmp_path, case, policy):
    from diffphys_amd import hip_backend

    key, bs, family, widths, want = case
    tpl, robot = _template(key, tmp_path)
    inp = _inputs(tpl, robot, bs, 60)
    for segw in widths:
        dm = hip_backend.DeviceModel(tpl)
        if segw is not None:
            dm.set_segment_width(segw)
        dm.set_kernel_family(family)
        dm.set_numeric_policy(hip_backend.NUM_LITERAL if policy == "literal" else hip_backend.NUM_STABLE)
        for loss in (False, True):
            # (the loss-evaluating forward exists wave-specialised only: the host sends it to the split kernel)
            want_l = ("split",) if loss and want == ("unsplit",) else want
            (a, info_a), (b, info_b) = _run_pair(dm, inp, dev, loss)
            assert info_a == info_b
            v = _variant(dm, info_b, family)
            assert v in want_l, (segw, loss, info_b, v)
            for k in a:
                assert torch.equal(a[k], b[k]) or bool(((a[k] == b[k]) | (torch.isnan(a[k]) & torch.isnan(b[k]))).all()), (segw, loss, k)
            print("%s bs=%d segw=%s loss=%d policy=%s: %s, bit-identical" % (key, bs, segw, loss, policy, v))
            assert float(a["grf"].abs().max()) > 0.0, "contacts must be active"


SENTINEL = -12345.678


def _fenced(n, dev, pad=4096):
    """n floats inside a buffer of sentinels: (buffer, view of the n floats)"""
    buf = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.float32, device=dev)
    return buf, buf[pad: pad + n]


@pytest.mark.parametrize("key,bs,family", [("laikago", 512, 2), ("laikago", 4096, 0), ("human", 1024, 0), ("quad", 8192, 0),
                                           ("laikago_toes", 256, 0), ("laikago12k", 37, 2)])
def test_forward_only_writes_nothing_outside_its_outputs(dev, tmp_path, key, bs, family):
    """Every output of a forward-only launch (the plain and the loss entry) sits inside a larger buffer of sentinels: afterwards the
    sentinels are untouched and the outputs hold what the saving launch writes."""
    from diffphys_amd import hip_backend

    tpl, robot = _template(key, tmp_path)
    dm = hip_backend.DeviceModel(tpl)
    dm.set_kernel_family(family)
    T = 60
    inp = _inputs(tpl, robot, bs, T)
    f2s = list(inp["frame2step"])
    F, nb, N = len(f2s), dm.nb, bs * dm.nb
    t = dev_inputs(inp, dev)
    ref = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s)
    sizes = dict(wp_pos=F * N * 7, wp_vel=F * N * 6, grf=F * N * 6, jaf=F * N * 6)
    bufs = {k: _fenced(n, dev) for k, n in sizes.items()}
    out = dict(ws=None, wp_pos=bufs["wp_pos"][1].view(F, N, 7), wp_vel=bufs["wp_vel"][1].view(F, N, 6), grf=bufs["grf"][1].view(F, N, 6),
               jaf=bufs["jaf"][1].view(F, N, 6))
    dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s, out=out, save_trajectory=False)
    torch.cuda.synchronize()
    for i, k in enumerate(("wp_pos", "wp_vel", "grf", "jaf")):
        buf, view = bufs[k]
        pad = (buf.numel() - view.numel()) // 2
        assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + view.numel():] == SENTINEL).all()), k
        assert torch.equal(view.view_as(ref[i]), ref[i]), k
    # the loss entry, through the C ABI with fenced outputs and NULL workspace / seeds
    lib = hip_backend.lib()
    rng = np.random.RandomState(4)
    tgt = torch.from_numpy((rng.randn(bs, F, nb, 7) * 0.05).astype(np.float32)).to(dev)
    pos_l, _, _, _, _, tl_ref = dm.rollout_forward_traj_loss(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s, target_pos=tgt)
    lsz = dict(table=bs * F, reduced=4, scale=bs * F)
    lb = {k: _fenced(n, dev) for k, n in lsz.items()}
    bufs = {k: _fenced(n, dev) for k, n in sizes.items()}
    f2s_c = (ctypes.c_int * F)(*f2s)
    rc = lib.pd_rollout_forward_traj_loss(dm.h, bs, T, ctypes.c_float(inp["dt"]), *[t[k].data_ptr() for k in FWD], F, f2s_c, None,
                                          *[bufs[k][1].data_ptr() for k in ("wp_pos", "wp_vel", "grf", "jaf")], tgt.data_ptr(), None,
                                          ctypes.c_float(0.1), None, None, lb["table"][1].data_ptr(), lb["reduced"][1].data_ptr(),
                                          lb["scale"][1].data_ptr(), hip_backend._stream())
    assert rc == 0, lib.pd_last_error().decode()
    torch.cuda.synchronize()
    for k, (buf, view) in list(bufs.items()) + list(lb.items()):
        pad = (buf.numel() - view.numel()) // 2
        assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + view.numel():] == SENTINEL).all()), k
    for k in ("table", "reduced", "scale"):
        assert torch.equal(lb[k][1], tl_ref[k].reshape(-1)), k
    assert torch.equal(bufs["wp_pos"][1], pos_l.reshape(-1))


def test_no_grad_forward_warp_needs_no_workspace(dev):
    """Laikago 4096 envs x 10 000 steps, 11 frames: the saving forward needs 47.8 GB of workspace.  ForwardWarp.apply under no_grad
    raises the peak of allocated device memory by no more than its outputs + 256 MB, and its frames equal a saving launch's bit for bit."""
    from diffphys_amd import dp_model, hip_backend, robots, synth

    tpl = robots.load_template("laikago")
    bs, T0, R = 4096, 100, 100
    T = T0 * R
    dm = hip_backend.DeviceModel(tpl)
    assert dm.workspace_floats(bs, T) * 4 > 47e9
    free, _ = torch.cuda.mem_get_info()
    if free < 110e9:
        print("SKIP reason: %.1f GB free, the saving comparison launch needs ~70 GB" % (free / 1e9))
        pytest.skip("needs ~110 GB of free device memory")
    inp = synth.make_inputs(tpl, "laikago", bs=bs, nsteps=T0, seed=21, seqs=("mi-trot", "mi-spin"), penetration=0.003)
    t = dev_inputs(inp, dev)
    for k in ("torques", "res_f", "refs"):   # the 100-step controls, repeated over the 10 000 steps
        t[k] = t[k].repeat((R,) + (1,) * (t[k].dim() - 1)).contiguous()
    f2s = list(range(0, T + 1, T // 10))
    h = warp_host("laikago", bs, T, f2s, inp["dt"], dev)
    args = [t[k] for k in synth.INPUT_NAMES]
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        pos, vel = dp_model.ForwardWarp.apply(*args, h)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    F, N = len(f2s), bs * dm.nb
    outputs = F * N * (7 + 6 + 6 + 6) * 4
    print("no-grad ForwardWarp: peak +%.1f MB, outputs %.1f MB, saving workspace %.1f GB" % (peak / 2**20, outputs / 2**20, dm.workspace_floats(bs, T) * 4 / 1e9))
    assert peak <= outputs + (256 << 20), (peak, outputs)
    grfs = [g.clone() for g in h.grfs]
    del h
    gc.collect()
    dm = hip_backend.device_model(warp_host("laikago", bs, T, f2s, inp["dt"], dev).env)   # the model ForwardWarp launched on
    pos_s, vel_s, grf_s, jaf_s, ws = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s)
    torch.cuda.synchronize()
    assert torch.equal(pos, pos_s) and torch.equal(vel, vel_s)
    assert all(torch.equal(grfs[f], grf_s[f]) for f in range(len(grfs)))


def test_a_rollout_the_saving_path_cannot_hold(dev):
    """Laikago, 262 144 envs (64 copies of 4 096 distinct ones) x 1 000 steps, frames every 100 steps: 306 GB of saving workspace, ~125 GB
    of inputs and outputs.  Forward-only, every copy reproduces the 4 096-env launch bit for bit."""
    from diffphys_amd import hip_backend, robots, synth

    free, _ = torch.cuda.mem_get_info()
    if free < 140e9:
        print("SKIP reason: %.1f GB of device memory free, the rollout needs ~125 GB" % (free / 1e9))
        pytest.skip("needs 140 GB of free device memory (%.1f GB free)" % (free / 1e9))
    tpl = robots.load_template("laikago")
    bs0, R, T0, RT = 4096, 64, 100, 10
    T = T0 * RT
    inp = synth.make_inputs(tpl, "laikago", bs=bs0, nsteps=T0, seed=22, seqs=("mi-trot", "mi-spin"), penetration=0.003)
    f2s = list(range(0, T + 1, 100))
    dm = hip_backend.DeviceModel(tpl)
    assert dm.workspace_floats(bs0 * R, T) * 4 > 300e9
    t0 = dev_inputs(inp, dev, FWD)
    for k in ("torques", "res_f", "refs"):
        t0[k] = t0[k].repeat((RT,) + (1,) * (t0[k].dim() - 1)).contiguous()
    pos0, vel0, grf0, jaf0, ws0 = dm.rollout_forward(bs0, T, inp["dt"], *[t0[k] for k in FWD], frame2step=f2s)
    assert float(grf0.abs().max()) > 1.0
    del ws0
    lead = dict(q_init=0, qd_init=0, torques=1, res_f=1, refs=1, target_ke=0, target_kd=0, body_inv_mass=0, body_inertia=0, body_inv_inertia=0)

    def tiled(k):
        x = t0[k]
        if lead[k]:
            return x.reshape(x.shape[0], bs0, -1).repeat(1, R, 1).reshape((x.shape[0], R * x.shape[1]) + tuple(x.shape[2:]))
        return x.reshape(bs0, -1).repeat(R, 1).reshape((R * x.shape[0],) + tuple(x.shape[1:]))

    t = {}
    for k in FWD:   # one at a time: the tiled controls are ~120 GB
        t[k] = tiled(k)
    bs = bs0 * R
    pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s, save_trajectory=False)
    torch.cuda.synchronize()
    assert ws is None
    del t
    for big, small in ((pos, pos0), (vel, vel0), (grf, grf0), (jaf, jaf0)):
        a = big.reshape(big.shape[0], R, -1)
        b = small.reshape(small.shape[0], 1, -1)
        assert bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_phys_model_eval_forward_is_forward_only_and_bit_identical(dev):
    """phys_model.forward() in eval mode: under no_grad the rollout takes the forward-only path (no trajectory, no seeds), with grad
    enabled the saving one -- the same loss values and side outputs bit for bit.  A training iteration afterwards (captured as one
    graph, as main.py runs it) still takes the saving path and back-propagates."""
    from diffphys_amd import hip_backend
    from test_gpu_workload import _model

    model, opts = _model("mi-pace", "fwdonly")
    model.reinit_envs(opts["num_envs"], frames_per_wdw=opts["frames_per_wdw"])
    calls = []
    orig = hip_backend.DeviceModel.rollout_forward_traj_loss

    def spy(dm, *a, **kw):
        calls.append(kw.get("save_trajectory", True))
        return orig(dm, *a, **kw)

    hip_backend.DeviceModel.rollout_forward_traj_loss = spy
    try:
        model.eval()
        fs = model.compute_frame_start()
        noise = model.make_q_init_noise()

        def run(grad):
            with torch.set_grad_enabled(grad):
                out = model.forward(frame_start=fs, q_init_noise=noise.clone() if noise is not None else None)
            side = dict(grfs=[g.detach().clone() for g in model.grfs], jafs=[g.detach().clone() for g in model.jafs],
                        sim=np.stack(list(model.sim_trajs)), info=model.traj_loss_info.detach().clone())
            return {k: v.detach().clone() for k, v in out.items()}, side

        a, sa = run(False)
        b, sb = run(True)
        assert calls == [False, True], calls
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]) or (bool(torch.isnan(a[k]).all()) and bool(torch.isnan(b[k]).all())), k
        assert all(torch.equal(x, y) for x, y in zip(sa["grfs"], sb["grfs"])) and len(sa["grfs"]) == len(sb["grfs"])
        assert all(torch.equal(x, y) for x, y in zip(sa["jafs"], sb["jafs"]))
        assert np.array_equal(sa["sim"], sb["sim"]) and torch.equal(sa["info"], sb["info"])
        # training afterwards: the captured iteration's rollout saves its trajectory and the parameters receive gradients
        model.train()
        del calls[:]
        assert model.capture_iteration(validate=True)
        out = model.iteration()
        assert calls and all(calls), calls
        assert torch.isfinite(out["total_loss"]).all()
        assert any(p.grad is not None and float(p.grad.abs().sum()) > 0 for p in model.parameters())
        model.update()
    finally:
        hip_backend.DeviceModel.rollout_forward_traj_loss = orig


def test_forward_only_refusals(dev):
    """A NULL workspace with seeds is refused with a message (the seeds serve an adjoint that cannot run); the adjoint entries keep
    refusing a NULL workspace."""
    from diffphys_amd import hip_backend, robots, synth

    tpl = robots.load_template("laikago")
    dm = hip_backend.DeviceModel(tpl)
    bs, T = 8, 10
    inp = synth.make_inputs(tpl, "laikago", bs=bs, nsteps=T, seed=1, steps_per_frame=5)
    t = dev_inputs(inp, dev)
    f2s = list(inp["frame2step"])
    F, nb = len(f2s), dm.nb
    lib = hip_backend.lib()
    e = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    pos, vel, grf, jaf = e(F, bs * nb, 7), e(F, bs * nb, 6), e(F, bs * nb, 6), e(F, bs * nb, 6)
    tgt, seed_pos, table, red, scale = e(bs, F, nb, 7), e(F, bs * nb, 7), e(bs, F), e(4), e(bs, F)
    f2s_c = (ctypes.c_int * F)(*f2s)
    for sp, sg in ((seed_pos, None), (None, seed_pos)):
        rc = lib.pd_rollout_forward_traj_loss(dm.h, bs, T, ctypes.c_float(inp["dt"]), *[t[k].data_ptr() for k in FWD], F, f2s_c, None,
                                              pos.data_ptr(), vel.data_ptr(), grf.data_ptr(), jaf.data_ptr(), tgt.data_ptr(), None,
                                              ctypes.c_float(0.1), None if sp is None else sp.data_ptr(), None if sg is None else sg.data_ptr(),
                                              table.data_ptr(), red.data_ptr(), scale.data_ptr(), hip_backend._stream())
        assert rc != 0
        assert "seed" in lib.pd_last_error().decode() and "workspace" in lib.pd_last_error().decode()
    # forward-only through the binding, then an adjoint on its (absent) workspace: refused by the library
    pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s, save_trajectory=False)
    assert ws is None
    ap, av = e(F, bs * nb, 7), e(F, bs * nb, 6)
    g = dm._alloc_grads(bs, T, dev)
    rc = lib.pd_rollout_backward(dm.h, bs, T, ctypes.c_float(inp["dt"]), *[t[k].data_ptr() for k in BWD], F, f2s_c, None, ap.data_ptr(),
                                 av.data_ptr(), *[g[k].data_ptr() for k in FWD], hip_backend._stream())
    assert rc != 0 and "null device pointer" in lib.pd_last_error().decode()
    with pytest.raises((TypeError, AttributeError, RuntimeError)):
        dm.rollout_backward(bs, T, inp["dt"], *[t[k] for k in BWD], f2s, ws, ap, av)
