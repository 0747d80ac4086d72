"""The boundary objects of oracle/_ref (the reference's fm.c, linear.c and packet.c compiled against the product's headers)
ask the dynamic linker for names.  Every one of them must be a name libka9q_hip.so exports (csrc/exports.map), or one of the
few the host side provides: examples/radio_threads.c for the demodulator threads, nothing for the packet decoder (its
capture file oracle/ref_packet_capture.c is linked into the object).  A name missing from the library fails here, on the
CPU, before anything is loaded next to a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"       # where oracle/Makefile looks for the reference tree

# what the host program defines for the object (radio.c:383 / audio.c:32,82 in the reference; examples/radio_threads.c here)
HOST = {"fm": {"compute_n0", "send_mono_output", "send_stereo_output"},
        "linear": {"compute_n0", "send_mono_output", "send_stereo_output"},
        "packet": set()}


def _exports():
    txt = open(os.path.join(ROOT, "ka9q_sdr_amd", "csrc", "exports.map")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    body = txt[txt.index("global:") + len("global:"):txt.index("local:")]
    return set(re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*;", body))


def _undefined(so):
    out = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True, check=True).stdout
    names = set()
    for ln in out.splitlines():
        f = ln.split()
        if len(f) < 2 or f[-2] in ("w", "v"):         # weak references (the C runtime's own hooks)
            continue
        if "@" in f[-1]:                              # versioned: glibc's
            continue
        names.add(f[-1])
    return names


@pytest.mark.parametrize("mode", ["fm", "linear", "packet"])
def test_dropin_object_binds_to_the_library(mode):
    so = os.path.join(ROOT, "oracle", "_ref", "libref_%s_dropin.so" % mode)
    if not os.path.exists(so):
        if not os.path.isdir(REFERENCE):
            pytest.skip("oracle/_ref/libref_%s_dropin.so not built and no reference tree to build it from" % mode)
        pytest.fail("the reference tree is present but build() did not make %s" % so)
    exports = _exports()
    assert {"create_filter_output", "execute_filter_output", "set_filter", "cnrmf"} <= exports
    need = _undefined(so)
    assert len(need) >= 8, need                        # the object does lean on the library
    host = need & HOST[mode]
    missing = need - exports - host
    assert not missing, "libref_%s_dropin.so needs names the library does not export: %s" % (mode, sorted(missing))
    # the harness that provides the host names really defines them
    src = open(os.path.join(ROOT, "examples", "radio_threads.c")).read()
    for n in sorted(host):
        assert re.search(r"^\w[\w \*]*\b%s\(" % n, src, flags=re.M), n
