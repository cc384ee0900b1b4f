"""What the host-side build tests share: the per-kernel report of one hipcc cross-compile per source (registers, spills,
occupancy, static LDS and scratch, the kernel's ISA, and where spill code sits relative to the MFMAs), the selector of a
source's wanted kernels, the template arguments of a mangled kernel name, and the reference-shaped C caller of
INTEGRATION.md section 1.  What is read out of a kernel's ISA lives in isa_analysis.py.  No GPU needed."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "cuda-winograd_amd", "csrc")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "cuda-winograd_amd")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


class _Kernel(dict):
    """One kernel's record.  The report is cached, so a record cannot be written to; it prints without its `body`."""

    def __repr__(self):
        return repr({k: v for k, v in self.items() if k != "body"})

    def _read_only(self, *args, **kwargs):
        raise TypeError("a kernel's record is shared by every test of the process: copy it to change it")

    __setitem__ = __delitem__ = __ior__ = update = setdefault = pop = popitem = clear = _read_only


@functools.lru_cache(maxsize=None)
def _compiled(src):
    """csrc/`src` is compiled once per process, in a directory of its own that goes when the process does."""
    tmp = tempfile.mkdtemp(prefix="build_report_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                          "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, src),
                          "-o", os.path.join(tmp, "x.o"), "-Rpass-analysis=kernel-resource-usage", "-save-temps"],
                         capture_output=True, text=True, timeout=600, cwd=tmp)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {"name": m.group(1)})
            continue
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"),
                         ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None and key not in cur:
                cur[key] = int(m.group(1))
    isa = [f for f in os.listdir(tmp) if f.endswith(".s") and "gfx950" in f]
    assert len(isa) == 1, isa
    with open(os.path.join(tmp, isa[0])) as f:
        text = f.read()
    for name, v in kernels.items():
        i = text.index(name + ":")
        body = text[i:text.index(".Lfunc_end", i)].splitlines()
        blocks, blk = [], []
        for line in body:
            if re.match(r"^\.LBB\d+_\d+:", line):
                blocks.append(blk)
                blk = []
            blk.append(line)
        blocks.append(blk)
        hot = [b for b in blocks if any("v_mfma" in x for x in b)]
        v["mfma"] = sum("v_mfma" in x for b in hot for x in b)
        v["spill_code_in_mfma_blocks"] = sum(any(p in x for p in ("v_readlane", "v_writelane", "scratch_load", "scratch_store"))
                                             for b in hot for x in b)
        desc = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\b(.*?)\.end_amdhsa_kernel", text, flags=re.S)
        assert desc, name
        v["static_lds"] = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc.group(1)).group(1))
        v["scratch"] = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc.group(1)).group(1))
        v["body"] = tuple(body)
    return {name: _Kernel(v) for name, v in kernels.items()}


def compile_report(src):
    """{mangled kernel name: record} of csrc/`src`.  A record holds `name`; from the compiler's resource remarks `vgprs`,
    `spill` and `sgpr_spill` (registers spilled), `occupancy` (waves per SIMD); from the kernel's descriptor `static_lds`
    and `scratch` (bytes per workgroup, per lane); `body`, the ISA lines from the kernel's label to its end; and from
    the body `mfma` (MFMAs in blocks that hold any) and `spill_code_in_mfma_blocks`."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return dict(_compiled(src))


def only(kernels, wanted):
    """{wanted: record}: each name of `wanted` is part of exactly one kernel's name, and the source compiled no other."""
    by = {want: [n for n in kernels if want in n] for want in wanted}
    assert all(len(v) == 1 for v in by.values()) and len(kernels) == len(wanted), sorted(kernels)
    return {want: kernels[name] for want, (name,) in by.items()}


def assert_no_spill_scratch_or_mfma(kernels):
    """What every kernel off the matrix pipe is held to; each record is printed (pytest -s)."""
    for name, v in sorted(kernels.items()):
        print(name, v)
        assert v["spill"] == 0 and v["sgpr_spill"] == 0 and v["scratch"] == 0, (name, v)
        assert v["mfma"] == 0, (name, v)


def template_args(name, family):
    """The template arguments (bools as 0 / 1) of `name` if it is a mangled instantiation of the kernel template
    `family`, else None.  The 1x1 kernels' last argument is their operand form AF (conv1x1_kernel.h)."""
    m = re.search(family + r"I((?:L[ib]\d+E)+)E", name)
    return [int(x) for x in re.findall(r"L[ib](\d+)E", m.group(1))] if m else None


# A caller shaped like the reference's Test.c:13-56 (own text): unprototyped use of the six entry
# points through the reference-named headers, `res >> 16` / `res & 0xFFFF`, first two calls
# discarded, integer means over nTest - 2.  The one edit INTEGRATION.md section 1 prescribes is made:
# cudaSetDevice(0) -> wino_set_device(0).
REFERENCE_SHAPED_CALLER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "Kernel128_one.h"
#include "Kernel128_winograd.h"
#include "Kernel256_one.h"
#include "Kernel256_winograd.h"
#include "util.h"
#include "winograd_mi355x.h"

int main(int argc, char** argv) {
  int nTest = 5, sum = 0, sum_other = 0, i, mode = 0;
  wino_set_device(0);
  if (argc >= 2) mode = atoi(argv[1]);
  if (argc >= 3) nTest = atoi(argv[2]);
  for (i = 0; i < nTest; i++) {
    int res = -1;
    printf("---- Iter: %d ----\n", i);
    switch (mode) {
      case 0: res = kernel_128(); break;
      case 1: res = kernel_256(); break;
      case 2: res = kernel_128_1_in(); break;
      case 3: res = kernel_128_1_out(); break;
      case 4: res = kernel_256_1_in(); break;
      case 5: res = kernel_256_1_out(); break;
    }
    if (i > 1) { sum += res >> 16; sum_other += res & 0xFFFF; }
  }
  printf("Average Total Time: [Mine: %d us], [cuDNN: %d us]\n", sum / (nTest - 2), sum_other / (nTest - 2));
  return 0;
}
"""


def build_reference_shaped_caller(workdir):
    """Compile + link per INTEGRATION.md section 1; returns the executable's path."""
    src = os.path.join(workdir, "RefShapedTest.c")
    with open(src, "w") as f:
        f.write(REFERENCE_SHAPED_CALLER)
    exe = os.path.join(workdir, "RefShapedTest")
    obj = os.path.join(workdir, "RefShapedTest.o")
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I" + INC, "-c", src, "-o", obj])
    subprocess.check_call(["gcc", "-o", exe, obj, "-L" + LIBDIR, "-lwinograd_mi355x",
                           "-Wl,-rpath," + LIBDIR, "-lpthread", "-lm"])
    return exe
