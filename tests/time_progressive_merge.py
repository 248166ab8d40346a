"""Manual timing (not collected by pytest) of the merge of progressive sessions; prints what profiles/progressive_merge_times.txt
records. HIP events (the library's own fold_ms), medians of 11 after a warm-up of every shape, cbox at 512x512, 1024x1024, 1280x720:
  * the fold launch (fold_kernel + finish_kernel, a GradPath pass that is not the first), as tests/time_progressive.py takes it;
  * the merge launch (merge_kernel + finish_kernel) in the same run: into a session that holds something (4 doubles read, 2 written
    per component: 6 against the fold's 5) and into an empty accumulator (the copy: 2 read, 2 written);
  * what a group pays per round to rebuild the total of three members on one device: three merges into an empty accumulator, their
    device time and the host wall time (each merge waits for its estimate).
    python tests/time_progressive_merge.py [--quick]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
dev = torch.device("cuda", 0)
torch.zeros(1, device=dev)
import gdpt_amd as G

quick = "--quick" in sys.argv
REPS = 3 if quick else 11
WARM = 2
HBM_PEAK = 8.0e12
XML = os.path.join(ROOT, "scenes", "cbox", "cbox_gdpt.xml")
med = lambda v: float(np.median(v))

for w, h in ((512, 512), (1024, 1024), (1280, 720)):
    sc = G.Scene(G.parse_scene(XML, film=(w, h)))
    ses = G.Progressive(sc, REPS + 3)
    for _ in range(3):                                   # warm-up: code objects, the first-pass variant, the planes
        ses.add_pass(1)
    fold = []
    for _ in range(REPS):
        ses.add_pass(1)
        fold.append(ses.status()["fold_ms"])
    ses.close()
    members = [G.Progressive(sc, 6, slice=(2 * i, 2)) for i in range(3)]
    for m in members:
        m.add_pass(1), m.add_pass(1)
    first, later, device, wall = [], [], [], []
    for r in range(WARM + REPS):
        acc = G.Progressive(sc, 6, slice=(0, 0))
        t0 = time.perf_counter()
        ms = [acc.merge(m)["fold_ms"] for m in members]
        t1 = time.perf_counter()
        acc.close()
        if r >= WARM:
            first.append(ms[0]); later += ms[1:]; device.append(sum(ms)); wall.append((t1 - t0) * 1e3)
    for m in members:
        m.close()
    sc.close()
    comp = w * h * 15
    f_ms, m_ms, c_ms = med(fold), med(later), med(first)
    tbs = lambda doubles, ms: comp * doubles * 8 / (ms * 1e-3) / 1e12
    print(f"{w}x{h}: fold {f_ms * 1e3:.1f} us (min {min(fold) * 1e3:.1f}, max {max(fold) * 1e3:.1f}; {tbs(5, f_ms):.2f} TB/s = {100 * tbs(5, f_ms) * 1e12 / HBM_PEAK:.0f} % of the HBM peak); "
          f"merge {m_ms * 1e3:.1f} us (min {min(later) * 1e3:.1f}, max {max(later) * 1e3:.1f}; {tbs(6, m_ms):.2f} TB/s = {100 * tbs(6, m_ms) * 1e12 / HBM_PEAK:.0f} %) = x{m_ms / f_ms:.2f} the fold; "
          f"merge into an empty accumulator {c_ms * 1e3:.1f} us ({tbs(4, c_ms):.2f} TB/s)", flush=True)
    print(f"{w}x{h}: rebuilding a three-member total: {med(device) * 1e3:.1f} us device time, {med(wall) * 1e3:.1f} us host wall "
          f"(min {min(wall) * 1e3:.1f}, max {max(wall) * 1e3:.1f})", flush=True)
