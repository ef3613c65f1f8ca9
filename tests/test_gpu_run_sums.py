"""The per-body run sums of the contact waves (csrc/pd_kernels.hip seg_run_sum) and the logged-hit pass around them: the adjoint's fast
path in both kernel families (13 values per hit) and the forward pass's RUNSUM hit pass (6 values per candidate).

Adjoint cases, Laikago, frames at states 1, 5, 9, 12 of 8 envs x 12 steps:
  flat   the penetration = 0.002 inputs of test_against_frozen_bits (seed 77): runs of one to three hits per foot
  tilt   the same robot tilted 0.05 rad about world x and dropped 4 mm into the ground: up to 11 hits per env-step, runs of 1 to 7 -- the
         first iteration, the second behind its wave-uniform test and the loop all run; chosen with the float64 oracle on the CPU
         (touch_fp32) so that 16 env-steps hold a run of >= 3 beside a run of exactly 1 and no env-step has more hits than a 16-lane
         segment; the test asserts both on the hit log the forward pass wrote
  idle   5 envs x 3 steps, states 1, 2, 3: the second wave has one env and three idle segments
Every gradient tensor of every case is held to the float64 C oracle with the project's rule for a change that may move roundings:
d_new <= max(2 d_parent, 1e-5), d = relmax(gradient, oracle), where d_parent was measured with the library of the commit before this change
on the same inputs (scripts/record_run_sums_fixture.py -> tests/golden/run_sums_parent.npz; never derived from the library under test).
Two runs give the same bits, and the selective launch (per-step gradients declined) gives the full launch's bits for what both return.
Quad-lane family: the forward outputs of `flat` are the parent build's bit for bit (same fixture), the gradients follow the same rule.

Forward RUNSUM: the instantiation is launched only when four env groups fill a workgroup, so 4096 envs x 6 steps (tilted 0.05 rad, dropped
3 mm -- at most 6 hits per env-step in the compared envs, so their candidates stay within a segment's lanes -- frame on the last state).  Eight envs spread over the batch must have the bits of the same envs run in a 64-env batch, which sums per body with
ds_add_f32; their hit log must hold a run of >= 3 and a run of 1."""
import functools
import os

import numpy as np
import pytest
import torch

from diffphys_amd import hip_backend, robots, synth
from gpu_harness import BWD, FWD, SEEDED, c_oracles, dev, dev_inputs, device_model  # noqa: F401
from helpers import GOLDEN, relmax

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "run_sums_parent.npz")
FRAME_OUT = ("wp_pos", "wp_vel", "grf", "jaf")
SEQS = ("mi-trot", "mi-spin")
# name -> (envs, steps, seeded states, steps_per_frame that makes synth draw that many seeds)
SHAPES = {"flat": (8, 12, [1, 5, 9, 12], 3), "tilt": (8, 12, [1, 5, 9, 12], 3), "idle": (5, 3, [1, 2, 3], 1)}
ADJOINT_RUNS = (("flat", 1), ("tilt", 1), ("idle", 1), ("flat", 2))   # (case, kernel family) the fixture holds distances for
TILT, DROP, RUNSUM_DROP = 0.05, 0.004, 0.003
SEGW = 16
BIG, SMALL, RUNSUM_STEPS = 4096, 64, 6


def qmul(a, b):   # (x, y, z, w)
    return np.array([a[3] * b[0] + b[3] * a[0] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + b[3] * a[1] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + b[3] * a[2] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def tilted(tpl, inp, drop):
    """the inputs with every root turned TILT about world x and lowered until its lowest contact point is `drop` under ground"""
    q = np.array(inp["q_init"], np.float64).reshape(-1, int(tpl["nq"])).copy()
    turn = np.array([np.sin(TILT / 2), 0.0, 0.0, np.cos(TILT / 2)])
    for e in range(len(q)):
        q[e, 3:7] = qmul(turn, q[e, 3:7])
    q[:, 1] -= synth.lowest_contact_y(tpl, q) + drop
    out = dict(inp)
    out["q_init"] = q.astype(np.float32).reshape(np.shape(inp["q_init"]))
    return out


def make_inputs(name, env_ids=None, steps=None):
    bs, T, states, spf = SHAPES[name]
    tpl = robots.load_template("laikago")
    ids = np.arange(bs) if env_ids is None else np.asarray(env_ids)
    if steps is not None:
        T, states, spf = steps, [steps], steps
    inp = synth.make_env_inputs(tpl, "laikago", ids, T, seed=77, steps_per_frame=spf, seqs=SEQS, penetration=0.0 if name == "tilt" else 0.002)
    assert len(inp["frame2step"]) == len(states)   # (the seeds were drawn for this many frames)
    inp["frame2step"] = list(states)
    return tpl, (tilted(tpl, inp, DROP if steps is None else RUNSUM_DROP) if name == "tilt" else inp)


@functools.lru_cache(maxsize=None)
def case(name):
    """(template, inputs, float64 oracle gradients) of an adjoint case: built once, shared, never written"""
    tpl, inp = make_inputs(name)
    _, g64 = c_oracles(tpl, inp, np.float64)
    return tpl, inp, g64


def hit_runs(dm, ws, bs, T):
    """the forward pass's hit log as scripts/gpu_hits.py reads it -> (counts [T, bs], run lengths per env-step: dict (step, env) -> list)"""
    raw = ws[T * 20 * bs * dm.nb:].view(torch.int32)[: T * bs * 32].view(T, bs, 32).cpu().numpy()
    cnt = raw[..., 0]
    runs = {}
    for s, e in zip(*np.nonzero(cnt > 0)):
        body = (raw[s, e, 1:1 + cnt[s, e]] >> 24) & 0x3f
        edges = np.flatnonzero(np.diff(body)) + 1
        runs[(int(s), int(e))] = np.diff(np.concatenate([[0], edges, [len(body)]])).tolist()
        assert len(set(body[np.concatenate([[0], edges])].tolist())) == len(edges) + 1, "a body's hits are contiguous"
    return cnt, runs


def launch(name, family, sel=False):
    """forward + adjoint of a case in one kernel family -> (frame outputs, gradients, hit counts, hit runs)"""
    tpl, inp, _ = case(name)
    dev = torch.device("cuda:0")
    dm = device_model(tpl, family=family)
    bs, T, f2s = np.asarray(inp["q_init"]).size // dm.nq, inp["nsteps"], list(inp["frame2step"])
    t = dev_inputs(inp, dev, SEEDED)
    pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=f2s)
    out = dict(zip(FRAME_OUT, (x.cpu().numpy() for x in (pos, vel, grf, jaf))))
    g = dm.rollout_backward(bs, T, inp["dt"], *[t[k] for k in BWD], f2s, ws, t["adj_pos"], t["adj_vel"], want=() if sel else hip_backend.GRAD_NAMES)
    torch.cuda.synchronize()
    cnt, runs = hit_runs(dm, ws, bs, T)
    return out, {k: v.cpu().numpy() for k, v in g.items()}, cnt, runs


run = functools.lru_cache(maxsize=None)(launch)


def distances(name, family):
    """relmax of every gradient tensor to the float64 oracle"""
    _, _, g64 = case(name)
    g = run(name, family)[1]
    for k in g:
        assert np.isfinite(np.asarray(g64[k])).all(), k
    return {k: relmax(g[k], np.asarray(g64[k], np.float64).reshape(g[k].shape)) for k in sorted(g)}


def record(path=FIXTURE):
    """What the fixture holds, measured with the library that is loaded: run this with the PARENT commit's build."""
    z = {"d/%s/%d/%s" % (name, family, k): np.float64(d) for name, family in ADJOINT_RUNS for k, d in distances(name, family).items()}
    z.update({"quad_flat/" + k: v for k, v in run("flat", 2)[0].items()})
    z["build_id"] = np.array(hip_backend.build_id())
    np.savez_compressed(path, **z)
    return z


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def check_gradients(name, family):
    fx, bad = fixture(), []
    g = run(name, family)[1]
    for k, d_new in distances(name, family).items():
        d_parent = float(fx["d/%s/%d/%s" % (name, family, k)])
        print("%-5s family %d %-16s d_parent %.3e  d_new %.3e" % (name, family, k, d_parent, d_new))
        if not (np.isfinite(g[k]).all() and d_new <= max(2.0 * d_parent, 1e-5)):
            bad.append((k, d_parent, d_new))
    assert not bad, bad


@pytest.mark.parametrize("name", ["flat", "tilt", "idle"])
def test_lane_per_body_adjoint(dev, oracle_libs, name):
    out, g, cnt, runs = run(name, 1)
    assert np.abs(out["grf"]).max() > 0, "something must touch"
    assert cnt.min() >= 0 and cnt.max() <= SEGW, "every env-step on the logged-hit fast path"
    if name == "tilt":
        assert any(max(r) >= 3 and 1 in r for r in runs.values()), "one env-step with a run of >= 3 and a run of 1"
        assert max(max(r) for r in runs.values()) >= 4, "the loop behind the two unrolled iterations must run"
    check_gradients(name, 1)
    again = launch(name, 1)
    for k in g:
        assert np.array_equal(again[1][k], g[k]), k
    part = launch(name, 1, sel=True)[1]
    assert set(part) == set(g) - set(hip_backend.GRAD_NAMES) and part
    for k in part:
        assert np.array_equal(part[k], g[k]), k


def test_quad_lane_adjoint(dev, oracle_libs):
    out, g, cnt, runs = run("flat", 2)
    fx = fixture()
    for k in FRAME_OUT:
        assert np.array_equal(out[k], fx["quad_flat/" + k].reshape(out[k].shape)), k
    assert cnt.min() >= 0 and max(max(r) for r in runs.values()) >= 2
    check_gradients("flat", 2)
    again = launch("flat", 2)
    for k in g:
        assert np.array_equal(again[1][k], g[k]), k


def test_forward_run_sums_have_the_atomic_path_bits(dev):
    tpl = robots.load_template("laikago")
    picked = np.linspace(0, BIG - 1, 8).astype(int)
    small_ids = np.concatenate([picked, np.setdiff1d(np.arange(SMALL + 8), picked)[: SMALL - 8]])
    res = {}
    for tag, ids in (("big", np.arange(BIG)), ("small", small_ids)):
        _, inp = make_inputs("tilt", env_ids=ids, steps=RUNSUM_STEPS)
        dm = device_model(tpl, family=1)
        bs, T = len(ids), RUNSUM_STEPS
        t = dev_inputs(inp, dev)
        pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=list(inp["frame2step"]))
        torch.cuda.synchronize()
        where = picked if tag == "big" else np.arange(8)
        cnt, runs = hit_runs(dm, ws, bs, T)
        res[tag] = dict(out={k: x.cpu().numpy().reshape(x.shape[0], bs, -1)[:, where] for k, x in zip(FRAME_OUT, (pos, vel, grf, jaf))},
                        cnt=cnt[:, where], runs=[r for (s, e), r in runs.items() if e in set(where.tolist())],
                        threads=dm.last_launch_info(0)["threads_per_wg"])
    # four env groups of a body, a contact and a cull wave each: the RUNSUM instantiation; the small batch's groups do not fill a workgroup
    assert res["big"]["threads"] == 4 * 192 and res["small"]["threads"] < 4 * 192, (res["big"]["threads"], res["small"]["threads"])
    assert np.array_equal(res["big"]["cnt"], res["small"]["cnt"])
    assert any(max(r) >= 3 for r in res["big"]["runs"]) and any(1 in r for r in res["big"]["runs"])
    for k in FRAME_OUT:   # (grf and jaf of the last state are zero: no step starts there; the contact wrenches act through the poses and twists)
        assert k in ("grf", "jaf") or np.abs(res["big"]["out"][k]).max() > 0, k
        assert np.array_equal(res["big"]["out"][k], res["small"]["out"][k]), k
