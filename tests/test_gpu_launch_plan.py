"""The host's launch plan, pinned: which kernel family, how many workgroups, threads, LDS bytes and envs per workgroup every rollout launch
gets (pd_last_launch_info), and which segment widths a model is refused at, with the refusal's text -- for the six models of
test_gpu_forward_only.CASES at every width, kernel family, numeric policy and a ladder of batch sizes either side of each threshold of
the plan (csrc/pd_host.hip plan_launch).  tests/golden/launch_plan.json was recorded by scripts/record_launch_plan.py from the library
as it was BEFORE the launch path was gathered into plan_launch; the same script's record_model() is replayed here, and every recorded
int and string must be equal.  Two-step rollouts of at most 4097 envs: about a second per model."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import record_launch_plan  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "launch_plan.json")) as _fh:
    FIXTURE = json.load(_fh)


def _leaves(tree, path=""):
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _leaves(tree[k], path + "/" + k)
    else:
        yield path, tree


def test_fixture_covers_every_model_and_case():
    assert sorted(FIXTURE["models"]) == sorted(record_launch_plan.MODELS)
    for key, rec in FIXTURE["models"].items():
        assert sorted(rec["widths"]) == sorted(str(w) for w in record_launch_plan.WIDTHS), key
        accepted = [w for w in rec["widths"].values() if "error" not in w]
        assert accepted, key
        n = len(record_launch_plan.FAMILIES) * len(record_launch_plan.POLICIES) * len(record_launch_plan.BATCHES)
        assert all(len(w["plans"]) == n and len(w["extra"]) == 4 for w in accepted), key


@pytest.mark.parametrize("key", record_launch_plan.MODELS)
def test_launch_plan_is_the_recorded_one(key, tmp_path):
    dev = torch.device("cuda:0")
    cus = int(torch.cuda.get_device_properties(dev).multi_processor_count)
    assert cus == FIXTURE["cu_count"], ("the launch plan is a function of the device's compute-unit count: the fixture was recorded on "
                                        "%d CUs, this device has %d" % (FIXTURE["cu_count"], cus))
    want = dict(_leaves(FIXTURE["models"][key]))
    got = dict(_leaves(record_launch_plan.record_model(key, dev, tmp_path)))
    assert sorted(got) == sorted(want)
    wrong = ["%s: recorded %r, now %r" % (k, want[k], got[k]) for k in sorted(want) if got[k] != want[k]]
    assert not wrong, "%d of %d entries differ:\n%s" % (len(wrong), len(want), "\n".join(wrong[:20]))
