#!/usr/bin/env python3
"""VGPRs / scratch / occupancy of every kernel in fcx_kernels.hip, fcx_kernels_wide.hip,
fcx_kernels_cr.hip, fcx_integrals.hip and fcx_atmos_terms.hip
(compiler remarks; a translation unit the checkout does not have is left out).

  python tools/kernel_resources.py [filter]
"""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
rows = []
for unit in ("fcx_kernels.hip", "fcx_kernels_wide.hip", "fcx_kernels_cr.hip", "fcx_integrals.hip",
             "fcx_atmos_terms.hip"):
    src = os.path.join(HERE, "..", "csrc", unit)
    if not os.path.exists(src):
        continue
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
               "-I" + os.path.join(HERE, "..", "csrc"), "-I" + os.path.join(HERE, "..", "..", "include"), "-c", src,
               "-o", os.path.join(tmp, "res.o"), "-Rpass-analysis=kernel-resource-usage"] + sys.argv[2:]
        out = subprocess.run(cmd, capture_output=True, text=True).stderr
    cur = None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"name": subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()}
            rows.append(cur)
            continue
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
flt = sys.argv[1] if len(sys.argv) > 1 else ""
for r in rows:
    if flt in r["name"]:
        print(f"{r.get('vgpr', '?'):>4} vgpr {r.get('scratch', '?'):>4} scratch {r.get('occ', '?'):>2} waves "
              f"{r.get('lds', 0):>6} lds  {r['name'].split('(')[0]}")
