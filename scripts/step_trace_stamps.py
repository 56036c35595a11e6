"""Stamps of the timed steps from a rocprofv3 kernel trace: tile / reduce averages, the gap from a
reduce's end to the next tile start, the tile-to-tile period, and how launches overlap."""
import csv
import statistics as st
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
ev = []
for r in rows:
    n = r["Kernel_Name"]
    k = "tile" if "sparse_tile_kernel" in n else "reduce" if "sparse_reduce_kernel" in n else None
    if k:
        ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), k, r.get("Queue_Id", ""), r.get("Stream_Id", "")))
ev.sort()
tiles = [e for e in ev if e[2] == "tile"]
reds = [e for e in ev if e[2] == "reduce"]
# the last 50 steps are the timed ones
tiles, reds = tiles[-50:], reds[-50:]
med = st.median
print("steps", len(tiles), len(reds), "queues of tile launches", sorted({t[3] for t in tiles}), "of reduces", sorted({r[3] for r in reds}))
print("tile us   avg %.2f med %.2f" % (st.mean((t[1] - t[0]) / 1e3 for t in tiles), med((t[1] - t[0]) / 1e3 for t in tiles)))
print("reduce us avg %.2f med %.2f" % (st.mean((r[1] - r[0]) / 1e3 for r in reds), med((r[1] - r[0]) / 1e3 for r in reds)))
per = [(b[0] - a[0]) / 1e3 for a, b in zip(tiles, tiles[1:])]
print("tile start to next tile start us: avg %.2f med %.2f min %.2f max %.2f" % (st.mean(per), med(per), min(per), max(per)))
gap = [(tiles[i + 1][0] - reds[i][1]) / 1e3 for i in range(len(tiles) - 1)]
print("reduce k end to tile k+1 start us: avg %.2f med %.2f" % (st.mean(gap), med(gap)))
ov = [max(0, tiles[i][1] - tiles[i + 1][0]) / (tiles[i + 1][1] - tiles[i + 1][0]) for i in range(len(tiles) - 1)]
print("fraction of tile k+1 inside tile k: avg %.3f med %.3f; starts before tile k ends: %d of %d" %
      (st.mean(ov), med(ov), sum(tiles[i + 1][0] < tiles[i][1] for i in range(len(tiles) - 1)), len(tiles) - 1))
inside = sum(tiles[i + 1][0] <= reds[i][0] and reds[i][1] <= tiles[i + 1][1] for i in range(len(tiles) - 1))
print("reduce k inside tile k+1's span: %d of %d" % (inside, len(tiles) - 1))
t2r = [(reds[i][0] - tiles[i][1]) / 1e3 for i in range(len(tiles))]
print("tile k end to reduce k start us: avg %.2f med %.2f" % (st.mean(t2r), med(t2r)))
print("span of the 50 steps us: %.1f -> %.2f a step" % ((reds[-1][1] - tiles[0][0]) / 1e3, (reds[-1][1] - tiles[0][0]) / 1e3 / len(tiles)))
