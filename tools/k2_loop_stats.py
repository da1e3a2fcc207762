#!/usr/bin/env python3
"""Static instruction counts of the ITEM LOOP of the weight-gradient kernels (csrc/txp_wgrad_bf16.hip), by class, from
   hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S social_stgcnn_amd/csrc/txp_wgrad_bf16.hip -o k2.s
   tools/k2_loop_stats.py k2.s
A kernel holds one item loop per layer kind (layer 0: c_in = 8, the others: c_in = 12): the natural loops of the control-flow
graph that contain a barrier and MFMAs.  Counted is every instruction of the loop's blocks, so the column tiles of BOTH
waves of a K-step where two share it (a wave issues only its own: 24 or 18 of the 42 MFMAs counted at c_in = 12, and one
operand read per tile).  No GPU needed."""
import collections
import re
import sys

lines = open(sys.argv[1]).read().split("\n")
starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*txp_wgrad_bf16_kernel\w*:", l)]
for i in starts:
    end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
    # basic blocks: [first line, last line], split at labels and behind branches
    heads = {i + 1}
    for j in range(i + 1, end):
        if re.match(r"^\.LBB\w+:", lines[j]):
            heads.add(j)
        if re.match(r"\s+s_(c?branch\w*|endpgm)\b", lines[j]):
            heads.add(j + 1)
    heads = sorted(h for h in heads if h < end)
    label_block = {}
    for b, h in enumerate(heads):
        m = re.match(r"^(\.LBB\w+):", lines[h])
        if m:
            label_block[m.group(1)] = b
    succ = collections.defaultdict(set)
    for b, h in enumerate(heads):
        last = (heads[b + 1] if b + 1 < len(heads) else end) - 1
        while last > h and not re.match(r"\s+[a-z]", lines[last]):
            last -= 1
        m = re.match(r"\s+(s_c?branch\w*)\s+(\.LBB\w+)", lines[last])
        if m:
            succ[b].add(label_block[m.group(2)])
        if not (m and m.group(1) == "s_branch") and "s_endpgm" not in lines[last] and b + 1 < len(heads):
            succ[b].add(b + 1)
    pred = collections.defaultdict(set)
    for b, ss in succ.items():
        for t in ss:
            pred[t].add(b)
    loops = {}
    for b, ss in succ.items():
        for t in ss:
            if t <= b:                                 # back edge b -> t: the natural loop with head t
                body, work = {t, b}, [b]
                while work:
                    x = work.pop()
                    if x == t:
                        continue
                    for p in pred[x]:
                        if p not in body:
                            body.add(p)
                            work.append(p)
                loops.setdefault(t, set()).update(body)
    print(lines[i].split(":")[0])
    best = {}                                          # (out-of-line blocks make larger "loops" around the item loop: keep
    for t, body in sorted(loops.items()):              # the smallest per MFMA count)
        c = collections.Counter()
        for b in body:
            for l in lines[heads[b]:heads[b + 1] if b + 1 < len(heads) else end]:
                m = re.match(r"\s+([a-z_0-9]+)", l)
                if not m:
                    continue
                op = m.group(1)
                cls = ("waitcnt" if op == "s_waitcnt" else "mfma" if op.startswith("v_mfma") else "lds" if op.startswith("ds_")
                       else "global" if op.startswith("global_") else "barrier" if op == "s_barrier"
                       else "valu" if op.startswith("v_") else "salu" if op.startswith("s_") else "other")
                c[cls] += 1
        if c["barrier"] and c["mfma"] and sum(c.values()) < sum(best.get(c["mfma"], {"x": 1 << 30}).values()):
            best[c["mfma"]] = c
    for n, c in sorted(best.items()):
        print("    item loop, %2d MFMAs: VALU %3d  SALU %3d  LDS %3d  global %2d  s_waitcnt %2d  s_barrier %d"
              % (n, c["valu"], c["salu"], c["lds"], c["global"], c["waitcnt"], c["barrier"]))
