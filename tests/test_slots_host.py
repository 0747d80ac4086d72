"""AddressSanitizer / UndefinedBehaviorSanitizer run of the slot banks' shared host layer (ka9q_sdr_amd/csrc/kq_slots.hpp and
kq::lazy_device of kq_host.hpp) on the CPU: a toy slot bank compiled against the device-less stand-in for the HIP runtime
(tests/tsan/slots_harness.cpp).  A set-up that fails at each of its runtime objects in turn must leave the handle holding
nothing, start over at the next set and leave nothing for the leak checker at destroy; the staging of a host-memory call,
the runs of active slots, the copy-back and the table's upload are checked against what kq_wfm / kq_rds / kq_fsk rely on.
A second toy bank with deferred slots and an event arena does the same for what kq_cw / kq_rtty rely on: set, remove and
reset without a device, the flush of mixed runs, a flush whose set-up fails at each object, the arena's entry points.
The GPU pool runs no sanitizers, so this is where the host layer's memory handling is checked."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_slot_host_layer_under_asan_and_ubsan():
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    probe = subprocess.run("echo 'int main(){}' | g++ -x c++ -fsanitize=address,undefined - -o /dev/null", shell=True,
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no AddressSanitizer / UndefinedBehaviorSanitizer runtime")
    tsan = os.path.join(HERE, "tsan")
    shutil.rmtree(os.path.join(tsan, "_build_slots"), ignore_errors=True)
    r = subprocess.run(["make", "-C", tsan, "slots"], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert "Sanitizer" not in out and "runtime error" not in out, out[-4000:]
    assert r.returncode == 0, out[-4000:]
    assert "slot banks' host layer: ok" in out
