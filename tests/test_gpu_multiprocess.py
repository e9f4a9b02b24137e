"""GPU parity -- several host threads, ranks and devices (row e); the plain-C host.
Tolerances and helpers: tests/gpu_common.py."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests.gpu_common import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu


def test_two_host_threads_on_two_streams():
    """ctypes releases the GIL, so two Python threads can be inside the library at once: enqueueing
    is serialised by the API lock and every stream has its own workspaces, so concurrent pipelines on
    different streams do not disturb each other."""
    import threading
    from scipy.signal import butter
    e = ext()
    sos = torch.from_numpy(butter(4, 0.1, output="sos"))
    K = 4097
    kf = (np.random.default_rng(1).standard_normal(K) / 64).astype(np.float32)
    xs = [dev(rnd((6, 300_000), 100 + i)) for i in range(2)]

    def run(x):
        y, _, _ = e.sos_forward(x, None, sos, None, None)
        y = e.fft_conv_forward(y, kf, (K - 1, 0))
        return e.normalize_forward(y, 0.5, e.STAT_RMS, False)

    refs = [run(x) for x in xs]
    torch.cuda.synchronize()
    outs, errs = [None, None], []

    def worker(i):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for _ in range(10):
                    outs[i] = run(xs[i])
            st.synchronize()
        except Exception as ex:  # pragma: no cover
            errs.append(ex)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert torch.equal(outs[i], refs[i]), i


def _sharded_hip_worker(rank, world, port, C, out_dir):
    """One of two ranks SHARING cuda:0 (the builder's lease is one GPU): real HIP kernels on this rank's
    rows, one gather over gloo (host-staged; on a multi-GPU node the same call is an RCCL gather)."""
    import os
    import sys

    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from torchfx_amd import distributed as D
        from torchfx_amd import filter as F
        torch.cuda.set_device(0)
        g = torch.Generator().manual_seed(0)
        x = torch.randn(C, 150_000, generator=g).to("cuda:0")
        pipe = [F.LoButterworth(2000, order=6), F.ParametricEQ(1000, 2.0, 3.0), F.FIR(np.hanning(301) / np.hanning(301).sum())]
        y = D.filter_sharded(pipe, x, 48000, gather=True)
        lo, hi = D.shard_bounds(C, world, rank)
        if rank == 0:
            assert y.is_cuda and y.shape == x.shape
            torch.save(y.cpu(), os.path.join(out_dir, "gathered.pt"))
        else:
            assert y is None
        yl = D.filter_sharded([F.HiButterworth(300, order=4)], x, 48000, gather=False)      # stateful lone IIR, rows stay local
        assert yl.is_cuda and yl.shape[0] == hi - lo
        torch.save(yl.cpu(), os.path.join(out_dir, f"local{rank}.pt"))
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_share_one_device_hip_kernels_sharded_and_gathered(tmp_path):
    import socket

    import torch.multiprocessing as mp
    from torchfx_amd import Wave
    from torchfx_amd import filter as F
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    C, world = 5, 2                                   # uneven blocks: 3 + 2 rows
    mp.spawn(_sharded_hip_worker, args=(world, port, C, str(tmp_path)), nprocs=world, join=True)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(C, 150_000, generator=g).to(DEV)
    one = (Wave(x, 48000, device=DEV) | F.LoButterworth(2000, order=6) | F.ParametricEQ(1000, 2.0, 3.0)
           | F.FIR(np.hanning(301) / np.hanning(301).sum())).ys
    y = torch.load(tmp_path / "gathered.pt")
    # the overlap-save pass packs two real frames (of neighbouring rows) into one complex transform, so a
    # row's float32 rounding noise depends on which row it is paired with: equal to one process within
    # the FFT tolerance, not bit for bit (the recursive kernel below is row-independent: bit-identical)
    close(y, one.cpu().numpy(), 2e-6, "sharded chain vs one process")
    loc = torch.cat([torch.load(tmp_path / f"local{r}.pt") for r in range(world)])
    assert torch.equal(loc, F.HiButterworth(300, order=4, fs=48000)(x).cpu())


def _sharded_rccl_worker(rank, world, port, C, out_dir):
    """One rank per GPU over backend "nccl" (= RCCL): uneven row blocks, the gather lands in row views of one
    preallocated output on the root, ranks_seen counts the ranks on the collective itself."""
    import os
    import sys

    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(rank)
    devr = torch.device("cuda", rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=devr)
    try:
        from torchfx_amd import distributed as D
        from torchfx_amd import filter as F
        assert D.ranks_seen(device=devr) == world
        g = torch.Generator().manual_seed(0)
        x = torch.randn(C, 150_000, generator=g).to(devr)
        pipe = [F.LoButterworth(2000, order=6), F.ParametricEQ(1000, 2.0, 3.0), F.FIR(np.hanning(301) / np.hanning(301).sum())]
        root = world - 1                                     # not rank 0: the root index is honoured
        out = torch.full((C, 150_000), float("nan"), device=devr) if rank == root else None
        y = D.filter_sharded(pipe, x, 48000, gather=True, dst=root, out=out)
        if rank == root:
            assert y is out and bool(torch.isfinite(out).all())
            torch.save(y.cpu(), os.path.join(out_dir, "gathered.pt"))
        else:
            assert y is None
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_sharded_over_rccl_on_two_or_more_devices(tmp_path):
    """VERDICT r2 #5c: `filter_sharded` over backend "nccl" with uneven blocks, one rank per device.  RCCL refuses two ranks on
    one device, so a one-device box runs a single rank: the RCCL communicator, ranks_seen over it and the gather into the
    root's preallocated output; with two or more devices the blocks are uneven and the root is not rank 0."""
    import socket

    import torch.multiprocessing as mp
    from torchfx_amd import Wave
    from torchfx_amd import filter as F
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    world = min(torch.cuda.device_count(), 4)         # with this process at most five processes hold a device
    C = 2 * world + 1                                 # uneven blocks
    mp.spawn(_sharded_rccl_worker, args=(world, port, C, str(tmp_path)), nprocs=world, join=True)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(C, 150_000, generator=g).to(DEV)
    one = (Wave(x, 48000, device=DEV) | F.LoButterworth(2000, order=6) | F.ParametricEQ(1000, 2.0, 3.0)
           | F.FIR(np.hanning(301) / np.hanning(301).sum())).ys
    close(torch.load(tmp_path / "gathered.pt"), one.cpu().numpy(), 2e-6, "RCCL-sharded chain vs one process")


def test_bench_two_ranks_on_one_device(tmp_path):
    """bench.py's N > 1 control flow (barrier, max over ranks, gather, value_with_gather, strong scaling)
    with the real kernels: two ranks on cuda:0, gloo for the collectives (TFX_BENCH_SHARE_DEVICE=1)."""
    import json
    import os
    import subprocess
    import sys
    import socket
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TFX_BENCH_SHARE_DEVICE="1")
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = str(sock.getsockname()[1])
    sock.close()
    for extra, scaling, chans in ((["--channels", "4"], "weak", 4), (["--scaling", "strong", "--total-channels", "6"], "strong", 3)):
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                            "127.0.0.1", "--master-port", port, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2",
                            "--warmup", "1", "--seconds", "30", "--gather"] + extra,
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["n_gpus"] == 2 and line["scaling"] == scaling and line["config"]["channels_per_gpu"] == chans
        assert line["value"] > 0 and 0 < line["value_with_gather"] < line["value"] and line["gather_ms"] > 0
        assert "cpu_baseline" not in line and "stages" not in line          # rank 0 at N = 1 only


def test_bench_plain_line_and_full_line(tmp_path):
    """A plain `python bench.py --gpus 1` prints the headline and nothing that needs runs of its own; --full adds the per-kernel
    table, the roofline and the N = 1 extras (the CPU baseline leg has its own test in test_bench_contract.py).  The output of
    the last timed step is the same either way."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    lines = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline"])):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--seconds", "2",
                            "--channels", "2", "--dump-outputs", str(tmp_path / name)] + extra,
                           env=env, capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines[name] = json.loads(out[0])
    plain, full = lines["plain"], lines["full"]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain and k in full
        if k not in ("value", "ms_per_step"):
            assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["steps"] == 2 and plain["warmup"] == 1 and plain["dump_outputs"]["file"] == "y.npy"
    moved = {"roofline", "kernels", "kernels_single_stream", "ms_per_step_with_event_profiling", "variants", "stages",
             "published_context", "cfg5_512ch_on_one_gpu", "cpu_baseline"}
    assert not moved & set(plain), moved & set(plain)
    assert moved - {"cpu_baseline"} <= set(full), moved - set(full)
    assert full["kernels"] and "iir_precision" in full["config"] and "cpu_baseline" not in full
    # every leg of --full ran: a leg that raises leaves an {"error": ...} entry (or a "skipped" one) instead of its figures
    legs = {"cfg5_512ch_on_one_gpu": full["cfg5_512ch_on_one_gpu"], **{f"published.{k}": v for k, v in full["published_context"]["cases"].items()},
            **{f"variants.{k}": v for k, v in full["variants"].items()},
            **{f"stages.{k}": v for k, v in full["stages"].items() if isinstance(v, dict)}}
    assert len(full["variants"]) == 3 and len(full["published_context"]["cases"]) == 7
    failed = {k: v for k, v in legs.items() if "error" in v or "skipped" in v}
    assert not failed, failed
    assert all("ms_per_step" in v for k, v in legs.items() if k.startswith(("variants.", "stages."))), legs
    assert full["cfg5_512ch_on_one_gpu"]["ms_per_step"] > 0 and full["roofline"]["step_frac"] > 0
    assert np.array_equal(np.load(tmp_path / "plain" / "y.npy"), np.load(tmp_path / "full" / "y.npy"))


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher in front (the shape of the command the driver uses at N = 1): bench.py
    re-executes itself under torch.distributed.run, one rank per GPU; rank 0 prints ONE JSON line with ranks_seen == 2.
    (TFX_BENCH_SHARE_DEVICE=1 puts both ranks on cuda:0 over gloo on a one-GPU box; never set by the driver.)"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["TFX_BENCH_SHARE_DEVICE"] = "1"
    for extra, scaling, chans in ((["--channels", "4", "--gather"], "weak", 4),
                                  (["--scaling", "strong", "--total-channels", "6"], "strong", 3)):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                            "--seconds", "30"] + extra, env=env, capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and len(line["devices"]) == 2
        assert {d["rank"] for d in line["devices"]} == {0, 1} and all(d["uuid"] for d in line["devices"])
        assert line["scaling"] == scaling and line["config"]["channels_per_gpu"] == chans and line["value"] > 0
        if "--gather" in extra:
            assert 0 < line["value_with_gather"] < line["value"]


def test_bench_starts_three_ranks_uneven_strong_split_and_gather():
    """the shape of a multi-GPU run -- `python bench.py --gpus N [--gather]` starts N ranks itself
    (share-device, gloo: one GPU here), 2 s signals; weak scaling, a strong split of N channels (one row per rank) and of N + 1
    (uneven: one rank holds two rows).  Rank 0 prints ONE line with value, value_with_gather, gather_ms, ranks_seen == N and
    N device records; a launcher whose world size disagrees with --gpus gets no line at all.
    N = 3: this process, the launcher and the ranks all open the one device, and a shared GPU takes at most six processes."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["TFX_BENCH_SHARE_DEVICE"] = "1"
    env["OMP_NUM_THREADS"] = "2"
    n = 3
    for extra, scaling, total, c0 in ((["--channels", "1"], "weak", n, 1),
                                      (["--scaling", "strong", "--total-channels", str(n)], "strong", n, 1),
                                      (["--scaling", "strong", "--total-channels", str(n + 1)], "strong", n + 1, 2)):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(n), "--steps", "2", "--warmup", "1",
                            "--seconds", "2", "--gather"] + extra, env=env, capture_output=True, text=True, timeout=900, cwd=root)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["n_gpus"] == n and line["ranks_seen"] == n and len(line["devices"]) == n
        assert {d["rank"] for d in line["devices"]} == set(range(n)) and all(d["uuid"] for d in line["devices"])
        assert line["distinct_device_uuids"] == 1                     # share-device mode: N ranks, one GPU (the driver's run: N)
        assert line["scaling"] == scaling and line["config"]["total_channels"] == total and line["config"]["channels_per_gpu"] == c0
        assert line["value"] > 0 and line["gather_ms"] > 0 and 0 < line["value_with_gather"] < line["value"]
    # the launcher's world size and --gpus disagree: nothing is printed
    import socket
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = str(sk.getsockname()[1]); sk.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", port, os.path.join(root, "bench.py"), "--gpus", "3", "--steps", "1", "--warmup", "0", "--seconds", "2"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode != 0 and not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_two_devices_in_one_process_keep_their_own_caches():
    """Every device-side cache is keyed by the device ordinal (plans, taps, spectra, scratch, internal streams):
    the same filters driven alternately on cuda:0 and cuda:1 from ONE process give the single-device results.
    With one visible device the same sequence runs on cuda:0 alone: the first call (cold caches) and every later
    one (warm caches) must agree bit for bit."""
    from scipy.signal import butter
    sos = torch.from_numpy(butter(6, 2000 / 24000, output="sos"))
    k = torch.from_numpy((np.hanning(513) / np.hanning(513).sum()).astype(np.float32))
    x = torch.from_numpy(rnd((4, 200_000), 41))
    ref = None
    second = "cuda:1" if torch.cuda.device_count() >= 2 else "cuda:0"
    for rep in range(2):
        for d in ("cuda:0", second, "cuda:0"):
            xd = x.to(d)
            y = ext().fft_conv_forward(ext().sos_forward(xd, None, sos, None, None)[0], k, (512, 0))
            yd = ext().fir_direct_forward(xd, k)
            out = torch.cat([y, yd]).cpu()
            if ref is None:
                ref = out
            assert torch.equal(out, ref), (rep, d)


def test_plain_c_host_filters_on_the_device(tmp_path):
    """examples/c_host.c --gpu: hipMalloc + tfx_sos_forward from C99, no torch in the process."""
    import subprocess
    from scipy.signal import sosfilt
    from tests.test_capi_exports import _build_c_host
    exe = _build_c_host(tmp_path, with_hip=True)
    out = subprocess.run([exe, "--gpu"], check=True, capture_output=True, text=True).stdout
    head = [float(v) for v in out.split("impulse response head:")[1].split()[:4]]
    sos = np.array([[0.0495329964, 0.0990659928, 0.0495329964, 1.0, -1.2796324250, 0.4777644106],
                    [1.0089, -1.9636, 0.9695, 1.0, -1.9636, 0.9784]])
    imp = np.zeros(8); imp[0] = 1.0
    np.testing.assert_allclose(head, sosfilt(sos, imp)[:4], rtol=0, atol=2e-6)
    # ... and tfx_sos_fft_conv_forward from C: the cascade inside the overlap-save pipeline with an identity FIR == the cascade kernel
    worst = float(out.split("fused cascade|identity FIR vs cascade: max difference")[1].split()[0])
    assert worst <= 2e-6, out
    # the workspaces of that step came from the allocator the C host installed (tfx_set_workspace_allocator) and went back to it
    calls, nbytes = (int(v) for v in out.split("workspaces through the host's allocator:")[1].replace(",", " ").replace(";", " ").split()[0:3:2])
    assert calls >= 1 and nbytes >= 8 << 20 and "after tfx_clear_caches: held 0" in out, out
