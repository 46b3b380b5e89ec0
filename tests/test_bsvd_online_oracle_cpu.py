"""CPU: the PyTorch restatement of the online BSVD machine (tests/bsvd_online_oracle.py) against the reference's own trace
(tests/golden/bsvd_online, recorded by tests/golden/make_golden_bsvd_online.py from ``BSVD.feedin_one_element``) and against the clip form
``oracle.nets.bsvd_seq`` - all bit for bit: every convolution sees one frame at a time in all three."""
import json
import os

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import weights as W
from oracle import nets as onets
from tests.bsvd_online_oracle import LAG, BsvdOnlineOracle
from tests.conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", "bsvd_online")
MANIFEST = json.load(open(os.path.join(GOLD, "MANIFEST.json")))


@pytest.fixture(scope="module")
def trace():
    return dict(np.load(os.path.join(GOLD, MANIFEST["bsvd32_online_16x24"]["file"])))


@pytest.fixture(scope="module")
def table():
    return W.bsvd_table(seed=21)


def test_fixture_is_listed_and_small():
    assert sorted(f for f in os.listdir(GOLD) if f.endswith(".npz")) == sorted(m["file"] for m in MANIFEST.values())
    for m in MANIFEST.values():
        assert os.path.getsize(os.path.join(GOLD, m["file"])) < 512 * 1024
        assert m["lag"] == LAG and m["oracle_maxdiff_vs_bsvd_seq"] == 0.0


def run(o, x, sched):
    outs, i = [], 0
    for n in sched:
        outs.append(o.push(torch.from_numpy(x[i:i + n].copy())))
        i += n
    assert i == x.shape[0]
    return outs


def test_restatement_equals_the_recorded_trace_and_the_clip(trace, table):
    x, y = trace["x"], torch.from_numpy(trace["y"])
    o = BsvdOnlineOracle(table)
    outs = run(o, x, [1] * x.shape[0])
    assert [t.shape[0] for t in outs] == [0] * LAG + [1] * (x.shape[0] - LAG)
    assert o.pending == LAG
    outs.append(o.flush())
    assert [bool(v) for v in trace["none"]] == o.last_none_log            # the None pattern, call by call
    got = torch.cat(outs)
    assert torch.equal(got, y)                                            # every output, bit for bit
    with torch.no_grad():
        assert torch.equal(got, onets.bsvd_seq(torch.from_numpy(x.copy())[None], table)[0])
    # a flush ends the stream: the next one is the recorded stream after reset()
    x2 = trace["x2"]
    got2 = torch.cat(run(o, x2, [2, 3]) + [o.flush()])
    assert [bool(v) for v in trace["none2"]] == o.last_none_log
    assert torch.equal(got2, torch.from_numpy(trace["y2"]))


@pytest.mark.parametrize("sched", [[4, 4, 4, 4, 4, 1], [1, 3, 2, 6, 5, 4], [21]], ids=lambda s: "-".join(map(str, s)))
def test_push_sizes_do_not_matter(trace, table, sched):
    o = BsvdOnlineOracle(table)
    outs = run(o, trace["x"], sched)
    done = np.cumsum(sched)
    assert [t.shape[0] for t in outs] == [int(max(0, d - LAG) - max(0, d - n - LAG)) for d, n in zip(done, sched)]
    assert torch.equal(torch.cat(outs + [o.flush()]), torch.from_numpy(trace["y"]))


def test_reset_in_mid_stream_and_short_streams(trace, table):
    o = BsvdOnlineOracle(table)
    run(o, trace["x"][:8], [4, 4])
    o.reset()
    assert o.pending == 0
    got = torch.cat(run(o, trace["x2"], [5]) + [o.flush()])
    assert torch.equal(got, torch.from_numpy(trace["y2"]))
    for frames in (1, 16, 17):
        x = trace["x"][:frames]
        got = torch.cat(run(o, x, [1] * frames) + [o.flush()])
        with torch.no_grad():
            assert torch.equal(got, onets.bsvd_seq(torch.from_numpy(x.copy())[None], table)[0]), frames
    assert o.flush().shape[0] == 0                                        # nothing pushed: nothing to drain
