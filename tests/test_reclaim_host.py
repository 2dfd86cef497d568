"""The plan gra_reclaim runs (gra::plan_reclaim, plain C++) on a CPU box:
scripts/test_reclaim_host.cpp is built with g++ -fsanitize=address,undefined
as its own program and driven over stdin. This file recomputes every
destination and the new cursor from the stated rule, checks the properties
the copy kernel relies on, and replays the plan's batches on a bytearray in
adversarial piece orders. Nothing expected comes from the code under test."""
import os
import random
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "build", "test_reclaim_host")
DIRECT, BOUNCE = 0, 1


@pytest.fixture(scope="module")
def driver():
    os.makedirs(os.path.join(REPO, "build"), exist_ok=True)
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "scripts/test_reclaim_host.cpp",
         "rocksplicator_amd/csrc/host_store.cpp", "-o", BIN],
        cwd=REPO, check=True)
    return BIN


def run_plan(driver, segs, used, bounce, piece):
    """-> None when the plan was refused, else a dict of the printed plan."""
    lines = [f"plan {used} {bounce} {piece} {len(segs)}"]
    lines += [f"{s} {n}" for s, n in segs]
    r = subprocess.run([driver], input="\n".join(lines) + "\n",
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout.splitlines()
    head = out[0].split()
    if head[0] == "err":
        assert len(out) == 1
        return None
    assert head[0] == "ok"
    cur, moved, bounced, ns, np_, nb = map(int, head[1:])
    assert len(out) == 1 + ns + np_ + nb
    S = [tuple(map(int, l.split()[1:])) for l in out[1:1 + ns]]
    P = [tuple(map(int, l.split()[1:])) for l in out[1 + ns:1 + ns + np_]]
    B = [tuple(map(int, l.split()[1:])) for l in out[1 + ns + np_:]]
    assert all(l[0] == "S" for l in out[1:1 + ns])
    assert all(l[0] == "P" for l in out[1 + ns:1 + ns + np_])
    assert all(l[0] == "B" for l in out[1 + ns + np_:])
    return dict(new_cursor=cur, bytes_moved=moved, bytes_bounced=bounced,
                segs=S, pieces=P, batches=B)


def pattern(n):
    """Position-dependent bytes: no two 8-B words of an arena are equal."""
    out = bytearray(n)
    for i in range(0, n, 8):
        out[i:i + 8] = ((i // 8 * 0x9E3779B97F4A7C15 + 0xABCDEF) &
                        ((1 << 64) - 1)).to_bytes(8, "little")
    return out[:n]


def check_plan(plan, segs, used, bounce, piece, rng):
    """Everything the issue states about a plan; returns the set of batch
    kinds it holds."""
    # destinations and cursor, recomputed from the rule
    want = []
    running = 0
    for src, n in sorted(segs):
        dst = running + (src - running) % 16
        want.append((src, n, dst))
        running = dst + n
    assert [(s, n, d) for s, n, d, _ in plan["segs"]] == want
    assert sorted(t for _, _, _, t in plan["segs"]) == list(range(len(segs)))
    for s, n, d, t in plan["segs"]:
        assert segs[t] == (s, n)  # tags carried through the sort
        assert d <= s and d % 16 == s % 16
    for (s0, n0, d0), (s1, n1, d1) in zip(want, want[1:]):
        assert d0 + n0 <= d1  # disjoint destinations
    assert plan["new_cursor"] == (running + 15) & ~15
    assert plan["new_cursor"] <= (used + 15) & ~15
    # pieces tile exactly the moved segments, in source order
    moved = [(i, s, n, d) for i, (s, n, d) in enumerate(want)
             if d != s and n]
    assert plan["bytes_moved"] == sum(n for _, _, n, _ in moved)
    pi = 0
    P = plan["pieces"]
    for i, s, n, d in moved:
        done = 0
        while done < n:
            seg, ps, pd, _, pn = P[pi]
            assert (seg, ps, pd) == (i, s + done, d + done)
            assert 0 < pn <= piece and pn % 8 == 0 and done + pn <= n
            done += pn
            pi += 1
    assert pi == len(P)
    # batches partition the pieces
    nxt = 0
    kinds = set()
    bounced = 0
    for kind, first, count, nbytes in plan["batches"]:
        assert first == nxt and count > 0
        nxt += count
        ps = P[first:first + count]
        assert nbytes == sum(p[4] for p in ps)
        kinds.add(kind)
        if kind == DIRECT:
            # no load of the batch can see a store of the batch
            assert max(p[2] + p[4] for p in ps) <= min(p[1] for p in ps)
        else:
            assert kind == BOUNCE
            assert nbytes <= bounce
            bounced += nbytes
            end = 0
            for _, src, _, bnc, n in ps:
                assert bnc >= end and bnc % 16 == src % 16
                end = bnc + n
            assert end <= bounce
    assert nxt == len(P)
    assert plan["bytes_bounced"] == bounced
    # the move itself, pieces of a batch reversed and shuffled
    orig = pattern(used)
    for order in ("reversed", "shuffled"):
        arena = bytearray(orig)
        for kind, first, count, _ in plan["batches"]:
            ps = P[first:first + count]
            ps = ps[::-1] if order == "reversed" else rng.sample(ps, len(ps))
            if kind == DIRECT:
                for _, src, dst, _, n in ps:
                    arena[dst:dst + n] = arena[src:src + n]
            else:
                buf = bytearray(bounce)
                for _, src, _, bnc, n in ps:  # fully out ...
                    buf[bnc:bnc + n] = arena[src:src + n]
                for _, _, dst, bnc, n in reversed(ps):  # ... then back
                    arena[dst:dst + n] = buf[bnc:bnc + n]
        for s, n, d in want:
            assert arena[d:d + n] == orig[s:s + n], (order, s, n, d)
    return kinds


def layout(rng, nseg, sizes):
    """Segments in source order, every src and size a multiple of 8: a first
    hole of 16 bytes (a gap below every piece size used here), small holes
    over the first third, then one hole of 30000 (a gap above every piece
    size) and holes of every size. -> (segments shuffled, used)"""
    segs, pos = [], 16
    for i in range(nseg):
        if i == nseg // 3:
            pos += 30000
        elif i:
            small = [0, 0, 0, 8, 16, 24]
            pos += rng.choice(small if i < nseg // 3
                              else small + [256, 4096, 30000])
        n = rng.choice(sizes)
        segs.append((pos, n))
        pos += n
    used = (pos + 15) & ~15
    rng.shuffle(segs)
    return segs, used


@pytest.mark.parametrize("seed", range(8))
def test_random_layouts(driver, seed):
    rng = random.Random(100 + seed)
    sizes = [24 * k for k in (1, 2, 3, 5, 40)] + [16, 32, 48, 400, 1024, 4096,
                                                 5000 * 8]
    segs, used = layout(rng, rng.randrange(20, 100), sizes)
    bounce, piece = rng.choice([(4096, 1024), (2048, 2048), (65536, 4096)])
    plan = run_plan(driver, segs, used, bounce, piece)
    assert plan is not None
    kinds = check_plan(plan, segs, used, bounce, piece, rng)
    assert kinds == {DIRECT, BOUNCE}  # small gaps first, then large ones


def test_everything_in_place(driver):
    rng = random.Random(1)
    segs = [(0, 48), (48, 24), (72, 24), (96, 160), (256, 1024)]
    plan = run_plan(driver, segs, 1280, 4096, 1024)
    assert check_plan(plan, segs, 1280, 4096, 1024, rng) == set()
    assert plan["pieces"] == [] and plan["bytes_moved"] == 0
    assert plan["new_cursor"] == 1280
    # an empty store
    plan = run_plan(driver, [], 0, 4096, 1024)
    assert plan["new_cursor"] == 0 and plan["batches"] == []
    # only the tail is dead: nothing moves, the cursor drops
    plan = run_plan(driver, segs[:3], 1280, 4096, 1024)
    assert check_plan(plan, segs[:3], 1280, 4096, 1024, rng) == set()
    assert plan["new_cursor"] == 96 and plan["bytes_moved"] == 0


@pytest.mark.parametrize("gap", [8, 16])
def test_small_gaps_bounce(driver, gap):
    """A gap smaller than any piece: every batch goes through the buffer. A
    gap of 8 in front of a 16-B aligned segment frees nothing (the segment
    stays), so the 8-B gap sits in front of a header array at 8 mod 16."""
    rng = random.Random(gap)
    if gap == 16:
        segs = [(0, 64), (80, 2000), (2080, 24 * 7), (2080 + 168, 4096)]
    else:
        segs = [(0, 64), (72, 24 * 3), (144, 2048), (2192, 24), (2216, 24)]
    used = (segs[-1][0] + segs[-1][1] + 15) & ~15
    plan = run_plan(driver, segs, used, 4096, 1024)
    kinds = check_plan(plan, segs, used, 4096, 1024, rng)
    if gap == 16:
        assert kinds == {BOUNCE} and plan["bytes_moved"] == 2000 + 168 + 4096
        assert len(plan["batches"]) >= 2  # more than one buffer's worth
    else:
        # 72 = 8 mod 16 cannot go to 64 = 0 mod 16: in place, like all after
        assert kinds == set() and plan["bytes_moved"] == 0
        assert plan["new_cursor"] == used


def test_single_headers_and_odd_header_arrays(driver):
    """24-byte segments (one header) and header arrays at src = 8 mod 16,
    behind gaps small and large."""
    rng = random.Random(7)
    segs, pos = [], 16
    for i in range(60):
        pos += (0, 16, 48, 2048)[i % 4] if i % 5 == 0 else 0
        n = 24 if i % 3 else 24 * (1 + i % 7)
        segs.append((pos, n))
        pos += n
    assert any(s % 16 == 8 for s, _ in segs)
    assert sum(n == 24 for _, n in segs) > 20
    used = (pos + 15) & ~15
    plan = run_plan(driver, segs, used, 4096, 1024)
    kinds = check_plan(plan, segs, used, 4096, 1024, rng)
    assert kinds == {DIRECT, BOUNCE}
    assert any(p[1] % 16 == 8 for p in plan["pieces"])


def test_segment_larger_than_the_bounce_buffer(driver):
    rng = random.Random(9)
    segs = [(0, 32), (64, 3 * 4096 + 8 * 5), (20000, 24)]
    used = 20032
    plan = run_plan(driver, segs, used, 4096, 1024)
    kinds = check_plan(plan, segs, used, 4096, 1024, rng)
    big = [b for b in plan["batches"] if b[0] == BOUNCE]
    assert len(big) >= 4 and BOUNCE in kinds
    assert plan["bytes_bounced"] >= 3 * 4096 + 40


def test_piece_of_16_bytes(driver):
    rng = random.Random(11)
    segs = [(0, 16), (40, 24 * 3), (128, 160), (1024, 24), (1048, 24 * 2),
            (4096, 512)]
    used = 4608
    plan = run_plan(driver, segs, used, 64, 16)
    kinds = check_plan(plan, segs, used, 64, 16, rng)
    # a gap is a positive multiple of 16, so it always holds a 16-B piece
    assert kinds == {DIRECT}
    assert len(plan["batches"]) > 10  # a gap of 16 holds one piece a batch
    assert max(p[4] for p in plan["pieces"]) == 16
    assert min(p[4] for p in plan["pieces"]) == 8  # the 8-B head


@pytest.mark.parametrize("case", ["overlap", "contained", "past_used",
                                  "odd_src", "odd_len", "piece_15",
                                  "bounce_lt_piece", "piece_0"])
def test_bad_input_is_refused(driver, case):
    used, bounce, piece = 4096, 4096, 1024
    segs = [(0, 64), (128, 256), (1024, 512)]
    if case == "overlap":
        segs.append((376, 64))
    elif case == "contained":
        segs.append((1040, 16))
    elif case == "past_used":
        segs.append((4000, 104))
    elif case == "odd_src":
        segs.append((2052, 16))
    elif case == "odd_len":
        segs.append((2048, 12))
    elif case == "piece_15":
        piece = 1000
    elif case == "bounce_lt_piece":
        bounce = 512
    elif case == "piece_0":
        piece = 0
    assert run_plan(driver, segs, used, bounce, piece) is None
    # the same input without the fault plans
    if case in ("overlap", "contained", "past_used", "odd_src", "odd_len"):
        assert run_plan(driver, segs[:3], used, bounce, piece) is not None
