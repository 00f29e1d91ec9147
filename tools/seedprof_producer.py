#!/usr/bin/env python3
"""Where the waves of the three-run seed kernel spend a group, consumer (seed_prof 1) and producer (seed_prof 2) side, for the three equal
runs (seed_prerun 0) and the pre-run window (seed_prerun 1), seed kernel alone and next to the trace kernel, on the headline workload.
The producer side answers how long a producer wave waits at barrier A — the slack the pre-run lives on — separately for the groups in
which the wave ran a chunk of the ahead pass and those in which it ran none.
usage: python tools/seedprof_producer.py [scene]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hanamaru-renderer_amd", "python"))
import hanamaru_amd as ha

CONSUMER = ["issue reg loads", "wait 16 regs", "window", "barrier B", "round + record", "ovf note", "barrier A"]
PRODUCER = ["window", "barrier B", "loads + ahead (+ pre-run)", "barrier A, chunk groups", "barrier A, idle groups"]
sc = ha.Scene(sys.argv[1] if len(sys.argv) > 1 else "rtcamp6_v3_1")
r = ha.Renderer(0)
r.upload_scene(sc)
r.set_resolution(1920, 1080)
for prerun in (0, 1):
    r.set_debug_option("seed_prerun", prerun)
    for label, skip in (("seed kernel alone", 16), ("next to the trace kernel", 0)):
        for prof in (1, 2):
            r.set_debug_option("seed_prof", 0)
            r.set_debug_option("debug_skip", 0)
            r.render(1, 9)
            r.synchronize()
            r.clear()
            r.set_debug_option("seed_prof", prof)
            r.set_debug_option("debug_skip", skip)
            a = r.stats()
            r.render(1, 33)
            r.synchronize()
            b = r.stats()
            ph = [y - x for x, y in zip(a["seed_phase_cycles"], b["seed_phase_cycles"])]
            groups = max(1, ph[7])
            ms = (b["seed_kernel_ms"] - a["seed_kernel_ms"]) / max(1, b["seed_launches"] - a["seed_launches"])
            print("seed_prerun %d, %s, %s waves: seed kernel %.2f ms per launch, %d wave-groups" % (prerun, label, "consumer" if prof == 1 else "producer", ms, groups))
            if prof == 1:
                for n, v in zip(CONSUMER, ph[:7]):
                    print("   %-28s %9.0f cycles per group" % (n, v / groups))
                print("   %-28s %9.0f cycles per group" % ("total", sum(ph[:7]) / groups))
            else:
                busy, idle = max(1, ph[5]), max(1, groups - ph[5])
                for n, v in zip(PRODUCER[:3], ph[:3]):
                    print("   %-28s %9.0f cycles per group" % (n, v / groups))
                print("   %-28s %9.0f cycles per such group (%d groups, %.1f %% of all)" % (PRODUCER[3], ph[3] / busy, ph[5], 100.0 * ph[5] / groups))
                print("   %-28s %9.0f cycles per such group" % (PRODUCER[4], ph[4] / idle))
                print("   %-28s %9.1f %% of the chunk groups" % ("wait at A < 4 init blocks", 100.0 * ph[6] / busy))
                print("   %-28s %9.0f cycles per group" % ("total", sum(ph[:5]) / groups))
r.set_debug_option("seed_prof", 0)
r.set_debug_option("debug_skip", 0)
r.close()
