"""What the host-side build tests share: the per-kernel resource report of a hipcc cross-compile (registers, spills,
occupancy, and where spill code sits relative to the MFMAs), the template arguments of a mangled kernel name, and the
reference-shaped C caller of INTEGRATION.md section 1.  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "cuda-winograd_amd", "csrc")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "cuda-winograd_amd")


def compile_report(src, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                          "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, src),
                          "-o", str(tmp_path / "x.o"), "-Rpass-analysis=kernel-resource-usage", "-save-temps"],
                         capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("spill", r"VGPRs Spill: (\d+)"),
                         ("sgpr_spill", r"SGPRs Spill: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None and key not in cur:
                cur[key] = int(m.group(1))
    isa = [f for f in os.listdir(tmp_path) if f.endswith(".s") and "gfx950" in f]
    assert len(isa) == 1, isa
    text = (tmp_path / isa[0]).read_text()
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
    return kernels


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
