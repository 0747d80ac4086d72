"""kq_fanout_* (include/ka9q_hip.h): the front-end fan-out a C host uses to shard channels over GPUs -- the
reference's UDP multicast (multicast.c:143-237) replaced by ncclBroadcast on a side stream, two slots.  One GPU is
all a test box has, so the communicator here has one rank; it still goes through librccl (ncclGetUniqueId,
ncclCommInitRank, ncclBroadcast on the side stream), the slot / event protocol is the one N ranks run, and the
batches come out of the bank equal to the oracle's.  The N-rank layout itself is covered on CPU
(tests/test_distributed_gloo.py) and measured by bench.py --gpus N."""
import ctypes as C

import numpy as np
import pytest
import torch

import ka9q_sdr_amd as kq
from common import bank_cfg, rel_rms, run_oracle
from ka9q_sdr_amd import workload as wl

pytestmark = pytest.mark.gpu


def test_fanout_of_one_through_rccl_feeds_a_bank(gpu):
    lib = kq.load_library()
    lib.kq_fanout_create.restype = C.c_void_p
    lib.kq_fanout_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.kq_fanout_post.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int]
    lib.kq_fanout_acquire.restype = C.c_void_p
    lib.kq_fanout_acquire.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_size_t)]
    lib.kq_fanout_release.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.kq_fanout_destroy.argtypes = [C.c_void_p]
    ident = C.create_string_buffer(128)
    assert lib.kq_fanout_unique_id(ident) == 0, lib.kq_last_error()
    assert any(ident.raw)

    g = dict(samprate=192000, L=512, M=513, D=4)
    fs, L, M = g["samprate"], g["L"], g["M"]
    plan = wl.channel_plan("cfg1", 2)
    nblocks, nbatches = 3, 4
    iq = wl.make_iq(fs, nbatches * nblocks * L, seed=77)
    want = run_oracle(plan, g, iq, nbatches * nblocks)

    stream = torch.cuda.Stream()
    bank = kq.Bank(fs, L, M, g["D"], len(plan), nblocks, stream=stream.cuda_stream)
    for p in plan:
        bank.add_channel(bank_cfg(p))
    nwin = (M - 1) + nblocks * L
    f = lib.kq_fanout_create(0, 0, 1, 0, ident, nwin)
    assert f, lib.kq_last_error()
    # a slot that has not been posted carries nothing; an oversized post is refused
    assert lib.kq_fanout_post(f, 0, None, nwin, 0) == -1
    hist = np.zeros(M - 1, np.complex64)
    got = [[] for _ in plan]
    windows = []
    for k in range(nbatches):          # window layout of kq_bank_process_resident: M-1 history + the batch's blocks
        batch = iq[k * nblocks * L:(k + 1) * nblocks * L]
        windows.append(np.ascontiguousarray(np.concatenate([hist, batch])))
        hist = batch[-(M - 1):]
    assert lib.kq_fanout_post(f, 0, windows[0].ctypes.data, nwin, 0) == 0     # prime: batch 0 travels
    for k in range(nbatches):
        slot = k & 1
        if k + 1 < nbatches:           # batch k+1 travels while batch k is processed
            assert lib.kq_fanout_post(f, slot ^ 1, windows[k + 1].ctypes.data, nwin, 0) == 0, lib.kq_last_error()
        n = C.c_size_t()
        p = lib.kq_fanout_acquire(f, slot, C.c_void_p(stream.cuda_stream), C.byref(n))
        assert p and n.value == nwin
        assert bank.process_resident(p, nblocks) == nblocks
        assert lib.kq_fanout_release(f, slot, C.c_void_p(stream.cuda_stream)) == 0
        bank.sync()
        for c in range(len(plan)):
            got[c] += [bank.audio(c, b) for b in range(nblocks)]
    for c in range(len(plan)):
        assert rel_rms(np.concatenate(got[c]), np.concatenate(want[c][0])) < 1e-5
    assert lib.kq_fanout_destroy(f) == 0
    bank.close()


def test_c_fanout_wrapper_stats_and_rccl_view(gpu):
    """ka9q_sdr_amd.shard.CFanout -- what bench.py --gpus N drives -- over a communicator of one: RCCL's own count of
    the world (ncclCommCount), its version, and the broadcasts timed on the side stream."""
    from ka9q_sdr_amd.shard import CFanout, share_unique_id
    lib = kq.load_library()

    def make_id():
        buf = C.create_string_buffer(128)
        assert lib.kq_fanout_unique_id(buf) == 0, lib.kq_last_error()
        return buf.raw

    ident = share_unique_id(make_id, 0)
    n = 4096
    fan = CFanout(lib, 0, 0, 1, n, ident)
    stream = torch.cuda.Stream()
    src = torch.arange(2 * n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for i in range(2):
        fan.fill(i, src.data_ptr())
    for k in range(6):
        i = k & 1
        p = fan.acquire(i, stream.cuda_stream)
        assert p
        fan.release(i, stream.cuda_stream)
        fan.post(i)
    st = fan.stats()
    assert st["world"] == 1 and st["rccl_ranks"] == 1 and st["rccl_version"] > 0, st
    # (a broadcast still in flight when its slot is posted again is not timed: at least the last two are)
    assert 2 <= st["broadcasts"] <= 8 and st["broadcast_ms"] > 0, st
    assert st["acquires"] == 6 and st["waits"] == 0 and st["wait_ms"] == 0, st      # waits are only timed on request
    # kq_fanout_enable_timing: an acquire that finds its batch still travelling records two events on the consumer's stream
    fan.enable_timing(True)
    for k in range(6, 12):
        i = k & 1
        assert fan.acquire(i, stream.cuda_stream)
        fan.release(i, stream.cuda_stream)
        fan.post(i)
    torch.cuda.synchronize()
    st = fan.stats()
    assert st["acquires"] == 12 and 0 <= st["waits"] <= 6 and st["wait_ms"] >= 0, st
    assert (st["waits"] == 0) == (st["wait_ms"] == 0), st
    fan.enable_timing(False)
    # the slot holds what the root put there
    back = torch.empty(2 * n, dtype=torch.float32, device="cuda")
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(back.data_ptr()), ctypes.c_void_p(fan.ptr[0]), ctypes.c_size_t(8 * n), 3) == 0
    torch.cuda.synchronize()
    assert torch.equal(back, src)
    fan.close()


def test_streaming_host_io_equals_the_blocking_calls(gpu):
    """kq_bank_push_iq_async / kq_bank_pull_planes_async (pinned host memory, copy streams) against kq_bank_push_iq /
    kq_bank_pull_audio / kq_bank_pull_status on the same input: same audio, same status, call after call."""
    g = dict(samprate=192000, L=512, M=513, D=4)
    fs, L, M = g["samprate"], g["L"], g["M"]
    plan = wl.channel_plan("cfg1", 3)
    plan[1] = dict(plan[1], demod="am", low=-5000.0, high=5000.0, recovery_rate=50.0)
    nblocks, ncalls = 4, 5
    iq = wl.make_iq(fs, ncalls * nblocks * L, seed=91)
    olen = L // g["D"]
    ref = kq.Bank(fs, L, M, g["D"], len(plan), nblocks, compute_n0=True)
    bank = kq.Bank(fs, L, M, g["D"], len(plan), nblocks, compute_n0=True)
    for p in plan:
        ref.add_channel(bank_cfg(p))
        bank.add_channel(bank_cfg(p))
    pinned = torch.from_numpy(iq.copy()).pin_memory()
    audio = [torch.zeros(len(plan) * nblocks * 2 * olen, dtype=torch.float32).pin_memory() for _ in range(2)]
    status = [torch.zeros(len(plan) * nblocks * C.sizeof(kq.ChanStatus), dtype=torch.uint8).pin_memory() for _ in range(2)]
    for k in range(ncalls):
        # queue call k (input copy, kernels, output copy) without waiting for call k - 1's copies
        bank.push_iq_async(pinned.data_ptr() + 8 * k * nblocks * L, nblocks * L)
        assert bank.process() == nblocks
        bank.pull_planes_async(audio[k & 1].data_ptr(), status[k & 1].data_ptr())
        ref.push_iq(iq[k * nblocks * L:(k + 1) * nblocks * L])
        assert ref.process() == nblocks
        bank.host_io_wait()
        a = audio[k & 1].numpy().reshape(len(plan), nblocks, 2 * olen)
        st = np.frombuffer(status[k & 1].numpy().tobytes(), dtype=np.dtype(kq.ChanStatus)).reshape(len(plan), nblocks)
        for c in range(len(plan)):
            for b in range(nblocks):
                want = ref.audio(c, b)
                assert np.array_equal(a[c, b, :len(want)], want), (k, c, b)
                ws = ref.status(c, b)
                assert st[c, b]["nout"] == ws["nout"] and st[c, b]["squelch_count"] == ws["squelch_count"]
                assert st[c, b]["bb_power"] == np.float32(ws["bb_power"]) and st[c, b]["n0"] == np.float32(ws["n0"])
    ref.close()
    bank.close()


def test_demodulator_stream_changes_from_call_to_call(gpu, monkeypatch):
    """The bank decides per call where the demodulators run: on the main stream, or (when the planes of the last call were
    pulled asynchronously, or the plan has AGC channels) on their own stream under the next filter pass.  FM-only plan,
    pulls on some calls and not on others, so that consecutive calls alternate between the two; every call's audio and
    status equal those of a bank that never overlaps (KQ_DEMOD_OVERLAP=0) and of one that always does (=1)."""
    g = dict(samprate=192000, L=512, M=513, D=4)
    fs, L, M = g["samprate"], g["L"], g["M"]
    plan = wl.channel_plan("cfg1", 4)
    nblocks, ncalls = 4, 9
    iq = wl.make_iq(fs, ncalls * nblocks * L, seed=93)
    olen = L // g["D"]
    banks = {}
    for name, env in (("auto", None), ("never", "0"), ("always", "1")):
        if env is None:
            monkeypatch.delenv("KQ_DEMOD_OVERLAP", raising=False)
        else:
            monkeypatch.setenv("KQ_DEMOD_OVERLAP", env)
        banks[name] = kq.Bank(fs, L, M, g["D"], len(plan), nblocks, compute_n0=True)
        for p in plan:
            banks[name].add_channel(bank_cfg(p))
    monkeypatch.delenv("KQ_DEMOD_OVERLAP", raising=False)
    pinned = torch.from_numpy(iq.copy()).pin_memory()
    audio = torch.zeros(len(plan) * nblocks * 2 * olen, dtype=torch.float32).pin_memory()
    status = torch.zeros(len(plan) * nblocks * C.sizeof(kq.ChanStatus), dtype=torch.uint8).pin_memory()
    pull_after = {1, 2, 4, 7}          # calls 2, 3, 5 and 8 then run overlapped in the "auto" bank, the others do not
    for k in range(ncalls):
        chunk = iq[k * nblocks * L:(k + 1) * nblocks * L]
        for name, bank in banks.items():
            if name == "auto":
                bank.push_iq_async(pinned.data_ptr() + 8 * k * nblocks * L, nblocks * L)
            else:
                bank.push_iq(chunk)
            assert bank.process() == nblocks
        pulled = None
        if k in pull_after:
            banks["auto"].pull_planes_async(audio.data_ptr(), status.data_ptr())
            banks["auto"].host_io_wait()
            pulled = audio.numpy().reshape(len(plan), nblocks, 2 * olen).copy()
        for c in range(len(plan)):
            for b in range(nblocks):
                want = banks["never"].audio(c, b)
                assert np.array_equal(banks["always"].audio(c, b), want), (k, c, b)
                assert np.array_equal(banks["auto"].audio(c, b), want), (k, c, b)
                if pulled is not None:
                    assert np.array_equal(pulled[c, b, :len(want)], want), (k, c, b)
                ws = banks["never"].status(c, b)
                for other in ("auto", "always"):
                    st = banks[other].status(c, b)
                    assert st["nout"] == ws["nout"] and st["squelch_count"] == ws["squelch_count"]
                    assert np.float32(st["bb_power"]) == np.float32(ws["bb_power"]) and np.float32(st["if_power"]) == np.float32(ws["if_power"])
    for bank in banks.values():
        bank.close()


def test_65536_points_with_forced_demodulator_overlap_and_streamed_planes(gpu, monkeypatch):
    """the four sibling workgroups of an N = 65536 channel-block wait for each other (bounded spin) and rely on
    being resident together; here they run with the last call's demodulators forced onto the second stream beside them
    (KQ_DEMOD_OVERLAP=1, which the bank itself never chooses at this size) and with the planes streamed out
    (kq_bank_pull_planes_async), six calls in a row without a host wait between the kernels.  Audio, n0 and the integer
    status must equal a bank that never overlaps, and kq_bank_host_io_wait must not report a lost sibling."""
    g = wl.GEOMETRY["cfg5"]
    fs, L, M, D = g["samprate"], g["L"], g["M"], g["D"]
    plan = wl.channel_plan("cfg5", 96)      # 384 sibling workgroups per block: most of the device's 512 slots
    nblocks, ncalls = 4, 6
    iq = wl.make_iq(fs, ncalls * nblocks * L, seed=93)
    olen = L // D
    monkeypatch.setenv("KQ_DEMOD_OVERLAP", "0")
    ref = kq.Bank(fs, L, M, D, len(plan), nblocks, compute_n0=True)
    monkeypatch.setenv("KQ_DEMOD_OVERLAP", "1")
    bank = kq.Bank(fs, L, M, D, len(plan), nblocks, compute_n0=True)
    monkeypatch.delenv("KQ_DEMOD_OVERLAP")
    for p in plan:
        ref.add_channel(bank_cfg(p))
        bank.add_channel(bank_cfg(p))
    pinned = torch.from_numpy(iq.copy()).pin_memory()
    audio = [torch.zeros(len(plan) * nblocks * 2 * olen, dtype=torch.float32).pin_memory() for _ in range(ncalls)]
    status = [torch.zeros(len(plan) * nblocks * C.sizeof(kq.ChanStatus), dtype=torch.uint8).pin_memory() for _ in range(ncalls)]
    bank.push_iq_async(pinned.data_ptr(), nblocks * L)
    for k in range(ncalls):      # the call order the header asks for: process k, push k + 1, pull k
        assert bank.process() == nblocks
        if k + 1 < ncalls:
            bank.push_iq_async(pinned.data_ptr() + 8 * (k + 1) * nblocks * L, nblocks * L)
        bank.pull_planes_async(audio[k].data_ptr(), status[k].data_ptr())
    bank.host_io_wait()          # raises if a sibling's word never arrived
    bank.sync()
    for k in range(ncalls):
        ref.push_iq(iq[k * nblocks * L:(k + 1) * nblocks * L])
        assert ref.process() == nblocks
        a = audio[k].numpy().reshape(len(plan), nblocks, 2 * olen)
        st = np.frombuffer(status[k].numpy().tobytes(), dtype=np.dtype(kq.ChanStatus)).reshape(len(plan), nblocks)
        for c in range(0, len(plan), 5):
            for b in range(nblocks):
                want = ref.audio(c, b)
                ws = ref.status(c, b)
                assert np.array_equal(a[c, b, :len(want)], want), (k, c, b)
                assert st[c, b]["nout"] == ws["nout"] and st[c, b]["hangcount"] == ws["hangcount"]
                assert st[c, b]["n0"] == np.float32(ws["n0"]) and not np.isnan(st[c, b]["n0"]), (k, c, b)
    ref.close()
    bank.close()


def test_process_spectrum_refuses_a_channel_with_its_own_oscillator(gpu):
    """kq_bank_process_spectrum serves what follows the master: a channel that still has a second LO to apply cannot be
    demodulated from a spectrum transformed elsewhere (radio.c:132-139 mixes in front of the master)."""
    g = dict(samprate=192000, L=512, M=513, D=4)
    bank = kq.Bank(g["samprate"], g["L"], g["M"], g["D"], 1, 1, compute_n0=True, fwd_mode=kq.KQ_FWD_FULL)
    bank.add_channel(bank_cfg(dict(demod="am", low=-5000.0, high=5000.0, second_lo=-20000.0, recovery_rate=50.0)))
    spec = torch.zeros(g["L"] + g["M"] - 1, dtype=torch.complex64, device="cuda")
    lib = kq.load_library()
    lib.kq_bank_process_spectrum.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
    assert lib.kq_bank_process_spectrum(bank.h, C.c_void_p(spec.data_ptr()), 1) == -1
    assert b"second LO" in lib.kq_last_error()
    bank.close()
    # without one it runs: an all-zero spectrum gives all-zero audio
    bank = kq.Bank(g["samprate"], g["L"], g["M"], g["D"], 1, 1, compute_n0=True, fwd_mode=kq.KQ_FWD_FULL)
    bank.add_channel(bank_cfg(dict(demod="linear", low=100.0, high=3000.0, second_lo=0.0, hangtime=1.1, recovery_rate=6.0)))
    assert lib.kq_bank_process_spectrum(bank.h, C.c_void_p(spec.data_ptr()), 1) == 1, lib.kq_last_error()
    assert not np.any(bank.audio(0, 0)) and bank.status(0, 0)["nout"] == g["L"] // g["D"]
    bank.close()


def test_push_iq_async_buffer_may_be_reused_after_two_more_pushes(gpu):
    """include/ka9q_hip.h's promise for kq_bank_push_iq_async: `iq` must stay unchanged until two more pushes have
    been queued -- so a host that rotates three pinned buffers and scribbles over the oldest as soon as the third push has
    returned must get the same audio as the blocking path.  Small blocks, many calls, no host wait in between: the host runs
    as far ahead of the device as the library lets it."""
    g = dict(samprate=192000, L=512, M=513, D=4)
    fs, L, M = g["samprate"], g["L"], g["M"]
    plan = wl.channel_plan("cfg1", 2)
    nblocks, ncalls = 4, 40
    iq = wl.make_iq(fs, ncalls * nblocks * L, seed=97)
    ref = kq.Bank(fs, L, M, g["D"], len(plan), nblocks, compute_n0=True)
    bank = kq.Bank(fs, L, M, g["D"], len(plan), nblocks, compute_n0=True)
    for p in plan:
        ref.add_channel(bank_cfg(p))
        bank.add_channel(bank_cfg(p))
    n = nblocks * L
    bufs = [torch.zeros(n, dtype=torch.complex64).pin_memory() for _ in range(3)]
    junk = torch.full((n,), 1e3 + 1e3j, dtype=torch.complex64)
    got = []
    for k in range(ncalls):
        bufs[k % 3].copy_(torch.from_numpy(iq[k * n:(k + 1) * n]))
        bank.push_iq_async(bufs[k % 3].data_ptr(), n)
        if k >= 2:
            bufs[(k - 2) % 3].copy_(junk)        # two more pushes have been queued since push k - 2: its buffer is ours again
        assert bank.process() == nblocks
        got.append([bank.audio(c, nblocks - 1).copy() for c in range(len(plan))] if k % 8 == 7 else None)
    bank.host_io_wait()
    for k in range(ncalls):
        ref.push_iq(iq[k * n:(k + 1) * n])
        assert ref.process() == nblocks
        if got[k] is not None:
            for c in range(len(plan)):
                assert np.array_equal(got[k][c], ref.audio(c, nblocks - 1)), (k, c)
    ref.close()
    bank.close()


def test_rccl_library_bound_is_the_one_torch_mapped(gpu):
    """kq_fanout_rccl_path: the shared object the fan-out's ncclBroadcast came from (dladdr).  In a process that also holds
    torch there are two candidates -- torch's own copy and /opt/rocm's -- and one process must not run two RCCLs: the path
    the library reports is one of the librccl objects mapped into this process, and exactly one is mapped."""
    lib = kq.load_library()
    ident = C.create_string_buffer(128)
    assert lib.kq_fanout_unique_id(ident) == 0          # loads librccl
    path = (lib.kq_fanout_rccl_path() or b"").decode()
    assert path and "rccl" in path, path
    mapped = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "librccl" in ln})
    import os
    assert os.path.realpath(path) in {os.path.realpath(m) for m in mapped}, (path, mapped)
    assert len({os.path.realpath(m) for m in mapped}) == 1, mapped


# cfg 5 with 16 channels x 4 blocks per rank: two PROCESSES share the one GPU here, and N = 65536's sibling workgroups wait for each
# other (kq_full16k.hip sibling_exchange) -- with both ranks' launches in flight at once every sibling has to fit on the device, or
# the two tenants starve each other's siblings until the bounded waits run out (minutes; the full 512 x 16 did exactly that).
@pytest.mark.parametrize("config,blocks,channels,total", [("cfg4", 64, 1024, 2048), ("cfg5", 4, 16, 32)])
def test_bench_launches_itself_as_two_ranks(gpu, config, blocks, channels, total):
    """`bench.py --gpus 2` as a FRESH child process (never an exec of this one): self_launch starts the two ranks through
    torch.distributed.run, rank 0's identifier travels over the process group, both ranks enter kq_fanout_create -- where
    RCCL itself refuses two ranks on one GPU, on every rank, so the all-or-nothing return and the ranks' fall-back
    agreement run on hardware -- the spin-up count is broadcast, the steps run on the torch twin over gloo and per_rank is
    gathered.  What the driver's 8-GPU run executes first is then not executed for the first time (VERDICT r4 #3a)."""
    import json
    import os
    import signal
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "6", "--spinup", "20",
           "--config", config, "--blocks", str(blocks), "--channels", str(channels),
           "--full", "--no-cpu-baseline", "--no-rows", "--no-realtime", "--no-host-io", "--no-second-row"]
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        out, err = p.communicate(timeout=420)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)       # the launcher and its ranks: exactly the group started here
        out, err = p.communicate()
        raise AssertionError("bench.py --gpus 2 did not finish: " + err[-2000:])
    assert p.returncode == 0, err[-3000:]
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 6 and d["scaling"] == "weak"
    assert d["config"]["channels_total"] == total and d["config"]["workload"].startswith(config)
    # RCCL carried nothing between the two ranks (one GPU): the line says that no scaling figure may be read off it
    assert d["scaling_measured"] is False and "host_ingest" not in d
    pr = d["per_rank"]
    assert [r["rank"] for r in pr] == [0, 1]
    for r in pr:
        assert r["ms_per_step"] > 0 and r["kernel_ms"] > 0 and r["diag_steps"] == 40
    rk = d["ms_per_step_ranks"]
    assert rk["min"] <= rk["max"] and abs(rk["max"] - d["ms_per_step"]) < 1e-3
    assert abs(max(r["ms_per_step"] for r in pr) - rk["max"]) < 0.02 * rk["max"] + 1e-3
    # two ranks on one GPU: RCCL refused the communicator on both, said so, and both took the torch twin
    assert d["fanout"].startswith("torch.distributed.broadcast (gloo)"), d["fanout"]
    assert "kq_fanout unavailable" in d["fanout"] and "ncclCommInitRank" in d["fanout"], d["fanout"]
    assert d["value"] > 0 and d["roofline"]["frac"] > 0


def test_bench_host_ingest_leg_on_one_gpu(gpu):
    """bench.py's `host_ingest` leg (at N > 1: the root takes every batch from pinned host memory and kq_fanout_post copies it
    into the slot and broadcasts it on the side stream -- H2D + ncclBroadcast + compute in one pipeline) run at N = 1 with
    `--ingest host`: the same code path with a world of one, so that the driver's 8-GPU run does not execute it for the
    first time."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "10", "--spinup", "40", "--ingest", "host",
           "--no-cpu-baseline", "--no-rows", "--no-realtime", "--no-host-io", "--no-second-row"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    hi = d["host_ingest"]
    # (a sanity bound, not a performance claim: ten steps on cold clocks, the H2D copy of the first batches not yet hidden --
    #  0.50-0.9 of the resident value by box)
    assert hi["steps"] == 10 and hi["value"] > 0.2 * d["value"] and hi["h2d_bytes_per_step"] == 8 * (8192 + 64 * 8192)
    assert d["scaling_measured"] is True and d["n_gpus"] == 1
