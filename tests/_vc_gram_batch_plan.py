"""The plan of a cdh_vc_gram_batch call (csrc/vc_gram_batch_types.hpp) restated in Python from the header's own constants, the
way `_vc_gram_numpy.launch` restates the single-point launch; tests/test_vc_gram_batch_host.py holds it to the compiled header."""
import os
import re

import _vc_gram_numpy as VG


def constants():
    txt = open(os.path.join(VG.CSRC, "vc_gram_batch_types.hpp")).read()
    out = {}
    for name in ("kVgbMaxPoints", "kVgbMaxGroupPoints", "kVgbTargetBlocks", "kVgbMinSharePoints"):
        out[name] = int(re.search(r"constexpr int64_t %s = (\d+);" % name, txt).group(1))
    for name in ("kVgbPartialDoubles", "kVgbOutDoubles"):
        out[name] = 1 << int(re.search(r"%s = \(int64_t\)1 << (\d+);" % name, txt).group(1))
    return out


K = constants()


def plan(n, Q, mb, m):
    """-> the regime, the workgroups per point G, the record length, the points of a full launch group, and per launch group
    its first point, its size, grid.y, the points per share and the shares' edges."""
    la, nrec = VG.launch(n, Q, mb), VG.nrec(Q, mb)
    G = la["G"]
    resident = la["chunks"] <= G
    pg = min(K["kVgbPartialDoubles"] // (G * nrec), K["kVgbOutDoubles"] // nrec, K["kVgbMaxGroupPoints"])
    groups = []
    for first in range(0, m, pg):
        pts = min(pg, m - first)
        if resident:
            shares = max(1, min(-(-K["kVgbTargetBlocks"] // G), pts // K["kVgbMinSharePoints"]))
            per = -(-pts // shares)
        else:
            per = 1
        gy = -(-pts // per)
        groups.append({"first": first, "pts": pts, "per": per, "grid_y": gy,
                       "edges": [min(pts, s * per) for s in range(gy + 1)]})
    return {"resident": resident, "G": G, "nrec": nrec, "group_points": pg, "groups": groups}


def rec_offset(n, Q, mb, point, block):
    return (point * VG.launch(n, Q, mb)["G"] + block) * VG.nrec(Q, mb)
