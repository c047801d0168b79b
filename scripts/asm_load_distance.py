#!/usr/bin/env python3
"""How far ahead of their waits the loads of a kernel's step loop are issued, in hipcc -S output.

  usage: asm_load_distance.py file.s <substring of the mangled kernel name>... [--waits]

The step loop is the longest backward-branch loop of the kernel.  Printed for it: vector, LDS-read, scalar-memory, vector-memory and scratch
instruction counts, and for every s_waitcnt that retires at least one load (LDS read or scalar load on lgkmcnt, buffer / global load on vmcnt)
the number of vector instructions of the wavefront between the LAST load it retires and the wait — the work that hides that load's round trip
without help from another wavefront.  The text is read top to bottom (forward branches inside the loop, such as the fold of a moving chain,
are walked as if taken in line).  --waits lists every such wait; the summary is always printed."""
import re
import sys

args = [a for a in sys.argv[1:] if not a.startswith("--")]
show = "--waits" in sys.argv
lines = open(args[0]).read().split("\n")
keys = args[1:]
start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and all(k in l for k in keys))
end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
body = lines[start:end + 1]
name = body[0].split(":")[0]
labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
loops = []
for i, l in enumerate(body):
    m = re.search(r"s_c?branch\w* (\.LBB\d+_\d+)", l)
    if m and m.group(1) in labels and labels[m.group(1)] < i:
        loops.append((i - labels[m.group(1)], labels[m.group(1)], i))
if not loops:
    sys.exit(f"{name}: no loop")
_, lo, hi = max(loops)
seg = [l.split(";")[0].strip() for l in body[lo:hi + 1]]
# the transition body: the loop's longest stretch without a label or a branch (what every transition executes, whatever the save rule and the fold do)
blocks, cur = [], []
for l in seg:
    if not l or l.startswith("."):
        if l.endswith(":"):
            blocks.append(cur); cur = []
        continue
    cur.append(l)
    if re.match(r"s_c?branch", l):
        blocks.append(cur); cur = []
blocks.append(cur)
tbody = max(blocks, key=len)
seg = [l for l in seg if l and not l.endswith(":") and not l.startswith(".")]
op = lambda l: l.split()[0]
is_valu = lambda l: op(l).startswith("v_")
is_ds_read = lambda l: op(l).startswith("ds_read") or op(l).startswith("ds_load")
is_ds = lambda l: op(l).startswith("ds_")
is_smem = lambda l: op(l).startswith("s_load") or op(l).startswith("s_buffer_load")
is_vmem = lambda l: re.match(r"(buffer|global|flat)_", op(l)) is not None
is_vload = lambda l: is_vmem(l) and ("load" in op(l) or "atomic" in op(l) and "glc" in l)

print(f"{name[:100]}")
res = {}
for l in lines[end:]:                      # the kernel's resource comments follow its code
    if (m := re.match(r"^; (NumVgprs|NumSgprs|ScratchSize|Occupancy): (\d+)", l)):
        res.setdefault(m.group(1), m.group(2))
    if len(res) == 4 or re.match(r"^_Z\w+:", l):
        break
print("  registers / scratch bytes / wavefronts per SIMD the registers allow: " + ", ".join(f"{k} {v}" for k, v in res.items()))
print(f"  step loop: {len(seg)} instructions; vector {sum(map(is_valu, seg))}, ds_read {sum(map(is_ds_read, seg))}"
      f" (b128 {sum(op(l) == 'ds_read_b128' for l in seg)}), scalar loads {sum(map(is_smem, seg))}, vector memory {sum(map(is_vmem, seg))},"
      f" scratch {sum(op(l).startswith('scratch_') for l in seg)}")

print(f"  transition body: {len(tbody)} instructions; vector {sum(map(is_valu, tbody))}, ds_read {sum(map(is_ds_read, tbody))}, scalar loads {sum(map(is_smem, tbody))},"
      f" vector memory {sum(map(is_vmem, tbody))}, scratch {sum(op(l).startswith('scratch_') for l in tbody)},"
      f" lane spills {sum(op(l) in ('v_readlane_b32', 'v_writelane_b32') for l in tbody)}")

valu = 0
lgkm, vm = [], []                  # outstanding operations in issue order: (kind, vector instructions issued before it, text)
waits = []                         # (kinds retired, distance of the last load retired, text of that load)
for l in seg:
    if is_valu(l):
        valu += 1
    elif is_ds(l):
        lgkm.append(("lds" if is_ds_read(l) else "other", valu, l))
    elif is_smem(l):
        lgkm.append(("smem", valu, l))
    elif is_vmem(l):
        vm.append(("vmem" if is_vload(l) else "other", valu, l))
    elif op(l) == "s_waitcnt":
        for cnt, q in (("lgkmcnt", lgkm), ("vmcnt", vm)):
            m = re.search(cnt + r"\((\d+)\)", l)
            if not m:
                continue
            n = int(m.group(1))
            # scalar loads return out of order: with one outstanding only lgkmcnt(0) retires anything for certain
            if cnt == "lgkmcnt" and n > 0 and any(k == "smem" for k, _, _ in q):
                continue
            done = q[:len(q) - n] if n < len(q) else []
            del q[:len(done)]
            loads = [d for d in done if d[0] != "other"]
            if loads:
                waits.append((sorted({d[0] for d in loads}), valu - loads[-1][1], loads[-1][2]))

for kind in ("lds", "smem", "vmem"):
    w = [d for ks, d, _ in waits if kind in ks]
    if w:
        print(f"  waits that retire a {kind} load: {len(w)}; vector instructions since the last load: mean {sum(w) / len(w):.1f}, min {min(w)},"
              f" max {max(w)}, at zero {sum(d == 0 for d in w)}, under 16: {sum(d < 16 for d in w)}")
    else:
        print(f"  waits that retire a {kind} load: 0")
if show:
    for ks, d, t in waits:
        print(f"    {'+'.join(ks):9s} {d:4d}   {t}")
