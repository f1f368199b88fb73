"""What the compiler made of the batched pass with the tall ZERO chains (kernels_fused_batch.hip,
CHAIN = 3, 4, 5), read from its gfx950 assembly, as test_fused_batch_zero_isa.py does for CHAIN = 2:
the transposed copy is streamed with non-temporal 16-byte loads, and what a form keeps per member - w
and t' (3), w alone (4), t' alone (5) - stays in registers: the widths of these forms
(ZeroTallWidthFor, ZeroTallHalfWidthFor) are chosen so that none spills to scratch.  Needs hipcc,
not a GPU."""

import os
import re
import shutil
import subprocess

import pytest

from epsilon_amd import build

KERNEL = "LassoBatchStreamKernel"
# the template arguments <T, NR, KB, GROUP = false, CHAIN = 3 | 4 | 5> in the mangled name
TALL_CHAIN = re.compile(r"%sI[fd]Li\d+ELi\d+ELb0ELi[345]EE" % KERNEL)


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.isabs(c) and os.path.exists(c):
            return c
    return None


def test_tall_chain_forms_keep_nontemporal_loads_and_no_scratch(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    flags = dict(build.DEVICE_SOURCES)["kernels_fused_batch.hip"]
    asm = tmp_path / "kernels_fused_batch.s"
    subprocess.run([hipcc] + build.COMMON + flags + ["-x", "hip", "--cuda-device-only", "-S",
                                                     os.path.join(build.CSRC, "kernels_fused_batch.hip"), "-o", str(asm)],
                   check=True, capture_output=True, text=True)
    text = asm.read_text()

    nt_loads = {}  # kernel symbol -> its non-temporal 16-byte loads
    for m in re.finditer(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)^\.Lfunc_end" % KERNEL, text, re.M | re.S):
        if not TALL_CHAIN.search(m.group(1)):
            continue
        code = [line.split(";")[0] for line in m.group(2).splitlines()]
        nt_loads[m.group(1)] = sum(1 for c in code if "global_load_dwordx4" in c and re.search(r"\bnt\b", c))
    scratch = {}   # kernel symbol -> private segment size (code object metadata)
    for m in re.finditer(r"^\s+\.name:\s+(_Z\w*%s\w*)\n(.*?)(?=^\s+- \.agpr_count|^\.\.\.)" % KERNEL, text,
                         re.M | re.S):
        if TALL_CHAIN.search(m.group(1)):
            scratch[m.group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", m.group(2)).group(1))

    assert nt_loads, "no tall-chain form of the batched pass found in the assembly"
    assert set(scratch) == set(nt_loads)
    for name in sorted(nt_loads):
        assert scratch[name] == 0, "%s uses %d bytes of scratch" % (name, scratch[name])
        assert nt_loads[name] >= 1, "%s has no non-temporal 16-byte load" % name
