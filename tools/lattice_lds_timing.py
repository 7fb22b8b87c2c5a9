#!/usr/bin/env python3
"""Device-event timings of the packed (LDS) form of both lattice field kernels, which tools/lattice_timing.py and
tools/lattice_gears_timing.py never reach (their maps are too large for it): small random-block maps with 2048 problems, 65 x 65
for the forward search and 45 x 45 with gears, and one 45 x 45 case that is wide by its counts.  Same calls and the same median
of 20 event-timed calls as those tools; the figures of profiles/lattice_field.txt.  Information, not a gate.

Usage:  python tools/lattice_lds_timing.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "pytorch-motion-planner_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import nfopp  # noqa: E402
from lattice_timing import lattice_calls  # noqa: E402
from lattice_gears_timing import gear_calls  # noqa: E402
from obstacle_map_timing import blob_map, timed  # noqa: E402

torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(77)
for side, calls, name in ((65, lambda lg, s, g: lattice_calls(lg, s, g, 0, "fixed"), "forward 65x65"),
                          (45, lambda lg, s, g: gear_calls(lg, s, g, (0, 0, 0)), "gears   45x45"),
                          (45, lambda lg, s, g: gear_calls(lg, s, g, (2, 1, 3)), "gears   45x45 costs (2,1,3)")):
    occ = blob_map(np.random.default_rng(side), side, 12, 3, 9) > 0
    grid = nfopp.OccupancyGrid(occ, (0.0, float(side), 0.0, float(side)), 1.0, device=dev)
    lg = nfopp.LatticeGrid.from_grid(grid)
    free = np.argwhere(~occ)
    pick = free[rng.integers(0, len(free), (2, 2048))]
    poses = [torch.tensor(np.concatenate([p[:, ::-1] + 0.5, rng.uniform(-np.pi, np.pi, (len(p), 1))], 1).astype(np.float32), device=dev)
             for p in pick]
    f, t, facts = calls(lg, poses[0], poses[1])
    tf, tt = timed(f, warmup=2, reps=20), timed(t, warmup=2, reps=20)
    print("  %-28s fields %9.3f  trace %8.3f   (%d goal states, %s form, %d of 2048 reached)"
          % (name, tf[0], tt[0], facts["goals"], facts["form"], facts["ok"]), flush=True)
