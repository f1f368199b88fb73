"""What the compiler made of the fused pass (kernels_fused.hip), read from its gfx950 assembly.

The pass streams the data matrix with non-temporal 16-byte loads so that it does not evict the
cached inverse from the Infinity Cache, and keeps everything else in registers.  Both properties
are the compiler's to drop: a guarded load rewritten as a select loses the `nt` modifier without
a word, a few more live values spill to scratch.  Needs hipcc, not a GPU."""

import os
import re
import shutil
import subprocess

import pytest

from epsilon_amd import build


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.isabs(c) and os.path.exists(c):
            return c
    return None


def test_fused_stream_kernels_keep_nontemporal_loads_and_no_scratch(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    flags = dict(build.DEVICE_SOURCES)["kernels_fused.hip"]
    asm = tmp_path / "kernels_fused.s"
    subprocess.run([hipcc] + build.COMMON + flags + ["-x", "hip", "--cuda-device-only", "-S",
                                                     os.path.join(build.CSRC, "kernels_fused.hip"), "-o", str(asm)],
                   check=True, capture_output=True, text=True)
    text = asm.read_text()

    nt_loads = {}  # kernel symbol -> its non-temporal 16-byte loads
    for m in re.finditer(r"^(_Z\w*LassoFusedStreamKernel\w*):[^\n]*\n(.*?)^\.Lfunc_end", text, re.M | re.S):
        code = [line.split(";")[0] for line in m.group(2).splitlines()]
        nt_loads[m.group(1)] = sum(1 for c in code if "global_load_dwordx4" in c and re.search(r"\bnt\b", c))
    scratch = {}   # kernel symbol -> private segment size (code object metadata)
    for m in re.finditer(r"^\s+\.name:\s+(_Z\w*LassoFusedStreamKernel\w*)\n(.*?)(?=^\s+- \.agpr_count|^\.\.\.)", text,
                         re.M | re.S):
        scratch[m.group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", m.group(2)).group(1))

    assert nt_loads, "no streaming kernel found in the assembly"
    assert set(scratch) == set(nt_loads)
    for name in sorted(nt_loads):
        assert scratch[name] == 0, "%s uses %d bytes of scratch" % (name, scratch[name])
        assert nt_loads[name] >= 1, "%s has no non-temporal 16-byte load" % name
    # exactly the forms of FusedPassExists (kernels.h), not the product of chains and heads
    assert len(nt_loads) == 120, (
        "%d streaming kernels, expected 120: with 256 threads 5 chunk counts x 9 forms (six chains with the zone or "
        "no head, the column chain with the ridge and the linear head, the tall chain with the cone) in f32 and in "
        "f64 = 90; with 512 threads 4 chunk counts (f32) + 2 (f64) x 5 forms (the first four chains, the column "
        "chain with the ridge head) = 30" % len(nt_loads))
