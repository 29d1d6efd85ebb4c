#!/usr/bin/env python3
"""Where the eight wavefronts of the helper-wave pair kernel's 512-thread workgroups land (libfabgpu_gputest.so gputest_wave_placement:
the HW_ID register of every wavefront of 235 such workgroups with the kernel's dynamic LDS): how often wavefront k and k + 4 share a SIMD.
One JSON line."""
import collections
import ctypes
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = ctypes.CDLL(os.path.join(ROOT, "fabric-mod_amd", "lib", "libfabgpu_gputest.so"))
WGS, LDS = 235, 160768          # the 30 000-tuple launch; kernels.hip pair_table_lds_bytes()
out = np.zeros(8 * WGS, np.uint32)
assert G.gputest_wave_placement(ctypes.c_uint32(WGS), ctypes.c_uint32(LDS), out.ctypes.data_as(ctypes.c_void_p)) == 0
hw = out.reshape(WGS, 8)
simd = (hw >> 4) & 3
cu = (hw >> 8) & 15
se_sh = hw >> 12
same_cu = bool(((cu == cu[:, :1]) & (se_sh == se_sh[:, :1])).all())
pairs = collections.Counter()
for g in range(WGS):
    for k in range(4):
        partner = [w for w in range(4, 8) if simd[g, w] == simd[g, k]]
        pairs["%d->%s" % (k, ",".join(map(str, partner)))] += 1
print(json.dumps({"workgroups": WGS, "all_waves_of_a_workgroup_on_one_cu": same_cu,
                  "wave_k_shares_simd_with_k_plus_4": float(np.mean(simd[:, :4] == simd[:, 4:])),
                  "simd_of_wave_0_to_7_first_wg": simd[0].tolist(), "pairings": dict(pairs)}))
