"""Walk the common path of the 16x16 screen body in a hipcc -S listing and count what stands between its MFMAs.

    python tools/body_asm_report.py coldrec_amd/lib/asm/score_topk_dma.s [usage.txt]

For each of the two M16 instantiations of score_topk_dma_kernel (compacted <...,true,true> and <...,false,true>) the tile loop is
found as the loop whose body holds the most v_mfma_f32_16x16x32_f16, and one trip (two tiles, 128 MFMAs) is walked from its
header along the path a tile without an event takes: the cheapest way through the loop's blocks from the header back to the
header that passes exactly 128 MFMAs (the event's path is longer, the exits never return).  Gap k of a tile is what stands
behind its MFMA k up to the next MFMA; what stands behind the last MFMA of a group (15, 31, 47, 63: the group's own last slot,
then waits, the barrier, tests and branches) is listed apart.  Reported for each of the trip's two tiles: s_nop on the path, the
instructions in gaps 16..21 (the head of the barrier group) and in the fullest gap, gaps 16..28 and the four group ends in
full; per trip: instructions, taken branches, and the spill traffic (v_readlane / v_writelane with a constant lane) on the path
and in the whole loop; and the FRAGMENT AUDIT: the body's counted waits name no register, so the listing is checked for an
instruction of the common path that reads or writes a register of a ds_read_b128 between that read and the s_waitcnt lgkmcnt(N)
that lands it (LDS operations complete in order: a wait leaves the N issued last in flight).  With a usage file (make asm writes one) the two kernels' resource lines are appended."""
import heapq
import re
import sys

MFMA = "v_mfma_f32_16x16x32_f16"
NAMES = {"Lb0ELb1ELb1E": "compacted <_Float16,128,4,false,true,true>", "Lb0ELb0ELb1E": "uncompacted <_Float16,128,4,false,false,true>"}


def instr(line):
    s = line.split(";")[0].strip()
    if not s or s.endswith(":") or s.startswith("."):
        return None
    return s


def kernel_lines(lines, key):
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*score_topk_dma_kernel\w*:", l) and key in l)
    end = next(i for i in range(start, len(lines)) if ".end_amdhsa_kernel" in lines[i] or lines[i].startswith("\t.section"))
    return lines[start:end]


def vregs(operand_text):
    """the VGPR numbers an operand text names (v7, v[10:13]; a[..] and s[..] are none)"""
    regs = set()
    for m in re.finditer(r"(?<![\w.])v(\d+)\b|(?<![\w.])v\[(\d+):(\d+)\]", operand_text):
        if m.group(1) is not None:
            regs.add(int(m.group(1)))
        else:
            regs.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return regs


def fragment_audit(path):
    """Walk the trip twice (the reads of one body are landed in the next) with the fragment registers in flight."""
    flying, bad, reads = [], [], 0          # flying: the destination sets of the LDS reads not yet landed, oldest first
    for lap in range(2):
        for _, s in path:
            op, _, rest = s.partition(" ")
            if op == "ds_read_b128":
                dst, addr = rest.split(",")[0], ",".join(rest.split(",")[1:])
                if vregs(addr) & set().union(*flying) if flying else False:
                    bad.append(s)
                flying.append(vregs(dst))
                reads += lap
            elif op == "s_waitcnt":
                m = re.search(r"lgkmcnt\((\d+)\)", rest)
                if m:
                    n = int(m.group(1))
                    flying = flying[len(flying) - n:] if n < len(flying) else flying
                    if n == 0:
                        flying = []
            elif op.startswith("ds_") or op.startswith("s_load") or op == "s_memtime":
                bad.append("another LGKM operation on the path, the count is off: " + s)
            elif flying and vregs(rest) & set().union(*flying):
                bad.append(s)
    if bad:
        return "fragment audit: FAILED, %d instructions touch a fragment register in flight (or upset the count): %s" % (len(bad), " | ".join(bad[:6]))
    return "fragment audit: %d fragment reads per trip, no instruction of the common path touches a fragment register between its read and the wait that lands it" % reads


def report(body, name):
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    # the tile loop's header: the depth-1 loop header with the most 16x16 MFMAs close behind it
    mf = [i for i, l in enumerate(body) if MFMA in l]
    heads = [i for l, i in labels.items() if "Loop Header: Depth=1" in body[i]]
    head = max(heads, key=lambda h: sum(1 for i in mf if h < i < h + 400))

    def nxt(i):
        """index of the first instruction at or behind line i"""
        while instr(body[i]) is None:
            i += 1
        return i

    # the cheapest way from the header back to the header that passes exactly 128 MFMAs (Dijkstra over (line, MFMAs passed), every
    # instruction costing one): the event's path is longer, the exits never return, a round through one body only passes 64
    start = (nxt(head), 0)
    best, prev, heap, goal = {start: 0}, {}, [(0, start)], None
    while heap:
        cost, (i, m) = heapq.heappop(heap)
        if cost > best[(i, m)] or cost > 1500:
            continue
        s = instr(body[i])
        if s.startswith("s_endpgm"):
            continue
        m2 = m + (1 if s.startswith(MFMA) else 0)
        if s.startswith("s_branch"):
            succ = [(labels[s.split()[1]], True)]
        elif s.startswith("s_cbranch"):
            succ = [(labels[s.split()[1]], True), (i + 1, False)]
        else:
            succ = [(i + 1, None)]
        for t, tk in succ:
            t = nxt(t)
            if t == start[0]:
                if m2 == 128:
                    goal = (i, m, tk)
                    heap = []
                    break
                continue
            if m2 > 128:
                continue
            if best.get((t, m2), 1 << 30) > cost + 1:
                best[(t, m2)] = cost + 1
                prev[(t, m2)] = (i, m, tk)
                heapq.heappush(heap, (cost + 1, (t, m2)))
    assert goal is not None, "no trip of 128 MFMAs found"
    steps, node, takens = [], goal[:2], {goal[:2]: goal[2]}
    while node != start:
        steps.append(node)
        pi, pm, ptk = prev[node]
        takens[(pi, pm)] = ptk
        node = (pi, pm)
    steps.append(start)
    steps.reverse()
    path, taken, n_mfma = [], 0, 0
    for node in steps:
        s = instr(body[node[0]])
        if s.startswith(("s_branch", "s_cbranch")):
            tk = takens[node]
            taken += 1 if tk else 0
            path.append(("br", s + ("   ; taken" if tk else "   ; falls through")))
        elif s.startswith(MFMA):
            n_mfma += 1
            path.append(("mfma", s))
        else:
            path.append(("i", s))
    assert n_mfma == 128, "a trip is two tiles of 64 MFMAs, walked %d" % n_mfma
    # gaps: gap k of a tile = what stands behind MFMA k (0..63) up to the next MFMA
    gaps, cur = [], None
    pre = []
    for kind, s in path:
        if kind == "mfma":
            cur = []
            gaps.append(cur)
        elif cur is None:
            pre.append(s)
        else:
            cur.append(s)
    gaps[-1].extend(pre)          # the head of the trip stands behind the even body's last MFMA
    tiles = [gaps[:64], gaps[64:]]
    print("== %s" % name)
    for t, tg in enumerate(tiles):
        nops = sum(1 for g in tg for s in g if s.startswith("s_nop"))
        outside = sum(len(tg[k]) for k in (15, 31, 47, 63))
        inside = [len(tg[k]) for k in range(64) if k not in (15, 31, 47, 63)]
        print("tile %d of the trip: s_nop %d, gaps 16..21 hold %s, fullest gap %d, behind the groups' last MFMAs (15/31/47/63) %s = %d" %
              (t, nops, [len(tg[k]) for k in range(16, 22)], max(inside), [len(tg[k]) for k in (15, 31, 47, 63)], outside))
        for k in range(16, 29):
            print("    gap %2d: %s" % (k, " | ".join(tg[k]) if tg[k] else "-"))
        for k in (15, 31, 47, 63):
            print("    behind MFMA %2d: %s" % (k, " | ".join(tg[k]) if tg[k] else "-"))
    print(fragment_audit(path))
    spill_path = sum(1 for _, s in path if s.startswith(("v_readlane", "v_writelane")))
    # the loop's extent: every block whose comment names this header (blocks of an out-of-line event may stand far behind the path)
    hid = body[head].split("BB")[1].split(":")[0]
    in_loop = [i for i in range(len(body)) if re.match(r"^\.LBB", body[i]) and ("Header=BB%s " % hid in body[i] or "Parent Loop BB%s " % hid in body[i])]
    spill_loop = 0
    n_loop = 0
    for b in in_loop + [head]:
        j = b + 1
        while j < len(body) and not re.match(r"^\.LBB", body[j]):
            s = instr(body[j])
            if s:
                n_loop += 1
                if s.startswith("v_readlane") and re.search(r", \d+$", s) or s.startswith("v_writelane") and re.search(r", \d+$", s):
                    spill_loop += 1
            j += 1
    print("per trip: %d instructions on the common path (%d MFMAs), %d taken branches; the loop holds %d instructions" % (len(path), n_mfma, taken, n_loop))
    print("spill traffic (v_readlane / v_writelane with a constant lane): %d on the common path, %d in the whole loop" % (spill_path, spill_loop))


def main():
    lines = open(sys.argv[1]).read().split("\n")
    for key, name in NAMES.items():
        report(kernel_lines(lines, key), name)
    if len(sys.argv) > 2:
        u = open(sys.argv[2]).read().split("\n")
        for i, l in enumerate(u):
            if "Function Name" in l and any(k in l for k in NAMES):
                key = next(k for k in NAMES if k in l)
                vals = [re.sub(r".*remark:\s*|\s*\[-Rpass.*", "", x) for x in u[i + 1:i + 10] if "remark:" in x and "Function Name" not in x]
                print("== resources, %s: %s" % (NAMES[key], "; ".join(v for v in vals if v.split(":")[0] in
                      ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill"))))


if __name__ == "__main__":
    main()
