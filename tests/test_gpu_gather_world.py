"""jb_comm_* / jb_gather_pcm with MORE THAN ONE rank, executed before the driver's 8-GPU node does (VERDICT r3
"next" 5): RCCL refuses two ranks on one device, so the ranks bind the test double of
tests/fake_rccl (the nine entry points jb_multi.cpp uses, over shared memory) through JB_RCCL_LIBRARY.  Fresh
child processes, no torch, at most four on the device.  Covered: the ncclAllGather of the ragged slab lengths,
the grouped ncclSend / ncclRecv, root != 0, a rank with an empty slab, 16-bit slabs, and the collective failure
semantics -- a rank without a batch, and f64 mixed with 16-bit slabs: EVERY rank gets an error, none hangs."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def double():
    r = subprocess.run(["bash", str(ROOT / "tests" / "fake_rccl" / "build.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip().splitlines()[-1]


def run_world(tmp_path, double, world, root, mode):
    env = dict(os.environ, JB_RCCL_LIBRARY=double, HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(ROOT / "tests" / "tools" / "gather_worker.py"), str(tmp_path),
                               str(world), str(r), str(root), mode], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()  # the exact children started here
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r}:\n{o}"
    return outs


@pytest.mark.parametrize("world,root,mode", [(4, 0, "f64"), (4, 2, "f64"), (3, 1, "i16"), (2, 0, "f64"),
                                             # an empty f64 batch on the root, 16-bit senders: not a mix,
                                             # and the receive slabs are sized by what the senders send
                                             (3, 1, "i16_f64_empty"), (3, 0, "i16_f64_empty")])
def test_gather_with_several_ranks_on_one_device(tmp_path, double, world, root, mode):
    outs = run_world(tmp_path, double, world, root, mode)
    assert all((tmp_path / f"done_{r}").read_text() == "ok" for r in range(world))
    assert f"(root): {world} slabs" in outs[root]


@pytest.mark.parametrize("world,root,mode", [(4, 0, "fail:3"), (3, 2, "fail:2"), (3, 0, "mixed")])
def test_a_failing_rank_fails_every_rank_and_hangs_none(tmp_path, double, world, root, mode):
    run_world(tmp_path, double, world, root, mode)
    assert all((tmp_path / f"done_{r}").read_text() == "error" for r in range(world))


def test_bench_rehearsal_line_is_self_verifying(double):
    """`bench.py --gpus 2` rehearsed on ONE device (JB_BENCH_REHEARSE=1, the test double as RCCL): the line must
    carry one identity record per rank -- the PCI bus id of its card and the communicator size RCCL itself reports
    (ncclCommCount through jb_comm_size) -- so that the driver's real N-GPU run proves by itself that N ranks ran
    on N distinct cards (VERDICT r5 "next" 7).  Here: two ranks, ONE card, size 2, and the gather keyed by its type;
    with --full, the config-3 job carries its own N = 1 reference."""
    import json

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(JB_BENCH_REHEARSE="1", JB_RCCL_LIBRARY=double, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--batch", "8", "--frames", "3000",
                        "--steps", "2", "--warmup", "1", "--utts", "64", "--gather", "--full", "--no-cpu-baseline"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["distinct_gpus"] == 1
    assert [x["rank"] for x in d["ranks"]] == [0, 1]
    assert all(x["comm_size_from_rccl"] == 2 for x in d["ranks"]), d["ranks"]
    assert d["ranks"][0]["pci_bus_id"] and d["ranks"][0]["pci_bus_id"] == d["ranks"][1]["pci_bus_id"]
    assert d["gather_dtype"] == "i16" and d["gather_i16_ms"] > 0
    strong, n1 = d["config3_strong"], d["config3_job_n1"]
    assert strong["value"] and n1["value"] and strong["speedup_over_n1"] == strong["value"] / n1["value"]
