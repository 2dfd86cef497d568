"""The ingest rule (gra::settle_group_locked over gra::roll_back_locked, plain
C++) on a CPU box: scripts/test_settle_host.cpp is built with
g++ -fsanitize=address,undefined as its own program and driven over stdin.
This file recomputes every printed line — the keep of each group and the seq
state of every shard after it — from the rule as it is stated, below in
Model.group. Nothing expected comes from the code under test.

The rule, per group of a finished tick, in tick order:
 - overflow, base_seq == 0 (real seqs start at 1; the tick found no room in
   the store): poison the shard, count a failure, roll back, keep nothing.
   Stated without "and the tick reported an error": k_scan2 raises the tick's
   error word in the statement that sets the overflow flag, and k_emit's
   descriptor blocks write base_seq == 0 exactly under that flag;
 - stale, the shard is already poisoned: roll back, keep nothing, durable_seq
   untouched;
 - clean, no validity bytes or every byte set: keep (n_entries, last_seq,
   whole), durable_seq = max(durable_seq, last_seq);
 - corrupt, first clear byte at update i: keep_recs = sum(counts[:i]),
   keep_seq = base_seq - 1 + keep_recs, keep (keep_recs, keep_seq, not whole),
   durable_seq = max(durable_seq, keep_seq), poison, count a failure, roll
   back.
Roll back: next_seq = durable_seq + 1, and the retained batches whose
base_seq lies past durable_seq leave the log from its end, log_used with
them."""
import os
import random
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "build", "test_settle_host")


@pytest.fixture(scope="module")
def driver():
    os.makedirs(os.path.join(REPO, "build"), exist_ok=True)
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "scripts/test_settle_host.cpp",
         "rocksplicator_amd/csrc/host_store.cpp", "-o", BIN],
        cwd=REPO, check=True)
    return BIN


class Shard:
    def __init__(self, durable=0, nxt=1, poisoned=0, log=()):
        self.durable, self.next, self.poisoned = durable, nxt, poisoned
        self.failures = 0
        self.log = list(log)  # (base_seq, count, rep_bytes)

    def line(self, i):
        return (i, self.durable, self.next, self.poisoned, self.failures,
                len(self.log), sum(n for _, _, n in self.log))

    def roll_back(self):
        self.next = self.durable + 1
        while self.log and self.log[-1][0] > self.durable:
            self.log.pop()


class Model:
    """A scenario: the input text as it grows and the lines it must print."""

    def __init__(self, shards):
        self.shards = shards
        self.text = ["scenario %d" % len(shards)]
        for sh in shards:
            self.text.append("%d %d %d %d" % (sh.durable, sh.next,
                                              sh.poisoned, len(sh.log)))
            self.text += ["%d %d %d" % ent for ent in sh.log]
        self.want = []

    def _state(self):
        self.want += [("S",) + sh.line(i) for i, sh in enumerate(self.shards)]

    def group(self, s, base_seq, counts, ok=None, n_entries=None,
              last_seq=None):
        """-> the keep (n_entries, last_seq, whole) the rule gives."""
        if n_entries is None:
            n_entries = sum(counts)
        if last_seq is None:
            last_seq = base_seq - 1 + n_entries if base_seq else 0
        self.text.append("group %d %d %d %d %d %d" % (
            s, base_seq, last_seq, n_entries, len(counts), ok is not None))
        self.text.append(" ".join(map(str, counts)))
        if ok is not None:
            self.text.append(" ".join(map(str, ok)))
        sh = self.shards[s]
        if base_seq == 0:  # overflow
            sh.poisoned = 1
            sh.failures += 1
            sh.roll_back()
            keep = (0, 0, 0)
        elif sh.poisoned:  # stale
            sh.roll_back()
            keep = (0, 0, 0)
        elif ok is None or all(ok):  # clean
            keep = (n_entries, last_seq, 1)
            sh.durable = max(sh.durable, last_seq)
        else:  # corrupt
            i = [bool(b) for b in ok].index(False)
            keep_recs = sum(counts[:i])
            keep = (keep_recs, base_seq - 1 + keep_recs, 0)
            sh.durable = max(sh.durable, keep[1])
            sh.poisoned = 1
            sh.failures += 1
            sh.roll_back()
        self.want.append(("K",) + keep)
        self._state()
        return keep

    def submit(self, s, count, rep_bytes):
        """-> the batch's base_seq."""
        sh = self.shards[s]
        base = sh.next
        self.text.append("submit %d %d %d" % (s, count, rep_bytes))
        sh.log.append((base, count, rep_bytes))
        sh.next += count
        self._state()
        return base

    def clear(self, s):
        self.text.append("clear %d" % s)
        self.shards[s].poisoned = 0
        self._state()


def check(driver, models):
    """One run of the driver over all the scenarios; every line compared."""
    text = "\n".join(l for m in models for l in m.text) + "\n"
    r = subprocess.run([driver], input=text, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [tuple([l.split()[0]] + [int(x) for x in l.split()[1:]])
           for l in r.stdout.splitlines()]
    want = [l for m in models for l in m.want]
    assert len(got) == len(want)
    for n, (g, w) in enumerate(zip(got, want)):
        assert g == w, (n, g, w)


def submit_group(m, s, counts, rep_bytes=40):
    """Batches of `counts` records submitted to shard s -> their base_seq."""
    bases = [m.submit(s, c, rep_bytes + 3 * i) for i, c in enumerate(counts)]
    return bases[0]


def test_overflow_group(driver):
    """Nothing kept; the shard is poisoned and rolled back to its durable
    boundary — with the tick's validity bytes and without."""
    models = []
    for ok in ([1, 1, 1], None):
        m = Model([Shard(durable=10, nxt=11, log=[(6, 5, 100)]), Shard()])
        submit_group(m, 0, [2, 1, 4])
        assert m.group(0, 0, [2, 1, 4], ok=ok, n_entries=0) == (0, 0, 0)
        sh = m.shards[0]
        assert (sh.durable, sh.next, sh.poisoned, sh.failures) == (10, 11, 1, 1)
        assert sh.log == [(6, 5, 100)]
        # still full at the next tick: one more failure, nothing else moves
        m.group(0, 0, [3], ok=[1], n_entries=0)
        assert (sh.durable, sh.next, sh.failures) == (10, 11, 2)
        assert m.shards[1].line(1) == Shard().line(1)
        models.append(m)
    check(driver, models)


def test_stale_group_on_a_poisoned_shard(driver):
    """durable_seq unchanged; the log pruned past it with log_used exact."""
    log = [(1, 3, 50), (4, 2, 70), (6, 1, 11), (7, 4, 90)]
    m = Model([Shard(durable=5, nxt=11, poisoned=1, log=log)])
    for ok in (None, [1, 1], [0, 1]):
        assert m.group(0, 7, [4, 2], ok=ok) == (0, 0, 0)
        sh = m.shards[0]
        assert (sh.durable, sh.next, sh.poisoned, sh.failures) == (5, 6, 1, 0)
        assert sh.log == log[:2] and sh.line(0)[-1] == 120
    check(driver, [m])


def test_first_update_bad(driver):
    """Nothing kept; durable_seq = base_seq - 1 unless it was already
    higher."""
    lo = Model([Shard(durable=3, nxt=4)])
    base = submit_group(lo, 0, [2, 3])
    assert base == 4
    # a seq hole below the group: the boundary moves up to base_seq - 1
    assert lo.group(0, 9, [2, 3], ok=[0, 1]) == (0, 8, 0)
    assert (lo.shards[0].durable, lo.shards[0].next) == (8, 9)
    assert lo.shards[0].log == [(4, 2, 40), (6, 3, 43)]
    hi = Model([Shard(durable=20, nxt=21)])
    assert hi.group(0, 9, [2, 3], ok=[0, 0]) == (0, 8, 0)
    sh = hi.shards[0]
    assert (sh.durable, sh.next, sh.poisoned, sh.failures) == (20, 21, 1, 1)
    check(driver, [lo, hi])


def test_bad_in_the_middle(driver):
    """Counts of 1, 0 and several: the clean prefix kept with its seq."""
    counts = [1, 0, 5, 1, 0, 3, 2]
    models = []
    for bad_at, recs in ((1, 1), (2, 1), (3, 6), (5, 7), (6, 10)):
        m = Model([Shard(durable=100, nxt=101)])
        base = submit_group(m, 0, counts)
        ok = [1] * len(counts)
        ok[bad_at] = 0
        if bad_at == 3:
            ok[5] = 0  # only the FIRST clear byte counts
        assert m.group(0, base, counts, ok=ok) == (recs, 100 + recs, 0)
        sh = m.shards[0]
        assert (sh.durable, sh.next, sh.poisoned) == (100 + recs, 101 + recs, 1)
        # the batches of the kept prefix stay retained, the rest leave
        assert [b for b, _, _ in sh.log] == \
            [101 + sum(counts[:i]) for i in range(len(counts))
             if 101 + sum(counts[:i]) <= 100 + recs]
        models.append(m)
    check(driver, models)


def test_second_group_of_a_shard_after_a_bad_first(driver):
    """Two groups of one shard in a tick, the first goes bad: the second is
    dropped whole, though every one of its own bytes is set."""
    m = Model([Shard(), Shard()])
    b0 = submit_group(m, 0, [2, 2, 2])
    b1 = submit_group(m, 1, [1])
    b2 = submit_group(m, 0, [3, 1])
    assert m.group(0, b0, [2, 2, 2], ok=[1, 0, 1]) == (2, 2, 0)
    assert m.group(1, b1, [1], ok=[1]) == (1, 1, 1)
    assert m.group(0, b2, [3, 1], ok=[1, 1]) == (0, 0, 0)
    assert m.shards[0].line(0) == (0, 2, 3, 1, 1, 1, 40)
    # the failure report clears the flag; the re-pull applies from seq 3
    m.clear(0)
    b = submit_group(m, 0, [2])
    assert b == 3 and m.group(0, b, [2]) == (2, 4, 1)
    check(driver, [m])


def test_clean_shard_beside_a_corrupt_one(driver):
    """A corrupt update in shard 1 leaves shards 0 and 2 of the same tick
    whole, before it and after it in tick order."""
    m = Model([Shard(durable=7, nxt=8), Shard(durable=1, nxt=2),
               Shard(durable=0, nxt=1, log=[])])
    bases = [submit_group(m, s, [1, 4, 2]) for s in range(3)]
    ok = {0: [1, 1, 1], 1: [1, 0, 1], 2: [1, 1, 1]}
    keeps = [m.group(s, bases[s], [1, 4, 2], ok=ok[s]) for s in range(3)]
    assert keeps == [(7, 14, 1), (1, 2, 0), (7, 7, 1)]
    for s in (0, 2):
        sh = m.shards[s]
        assert (sh.poisoned, sh.failures, len(sh.log)) == (0, 0, 3)
        assert sh.next == sh.durable + 1 == bases[s] + 7
    assert m.shards[1].line(1) == (1, 2, 3, 1, 1, 1, 40)
    check(driver, [m])


def test_clean_group_never_lowers_durable(driver):
    """A replayed tick: last_seq at or below durable_seq leaves it alone; a
    group of no records (LogData only) keeps nothing and still counts as
    clean."""
    m = Model([Shard(durable=50, nxt=51)])
    assert m.group(0, 10, [3, 3]) == (6, 15, 1)
    assert m.group(0, 51, [0, 0], ok=[1, 1]) == (0, 50, 1)
    assert m.shards[0].line(0) == (0, 50, 51, 0, 0, 0, 0)
    check(driver, [m])


def random_scenario(rng):
    nsh = rng.randrange(1, 5)
    shards = []
    for _ in range(nsh):
        durable = rng.choice([0, 0, rng.randrange(1, 1000), 1 << 40])
        log, seq = [], max(1, durable - rng.randrange(0, 12))
        for _ in range(rng.randrange(0, 6)):
            c = rng.choice([0, 1, 1, 2, 7])
            log.append((seq, c, rng.randrange(12, 300)))
            seq += c
        shards.append(Shard(durable, max(seq, durable + 1),
                            int(rng.random() < 0.15), log))
    m = Model(shards)
    for _ in range(rng.randrange(1, 5)):  # ticks
        failed = rng.random() < 0.5  # the tick's error word
        full = failed and rng.random() < 0.15
        groups = []
        for _ in range(rng.randrange(1, 7)):
            s = rng.randrange(nsh)
            counts = [rng.choice([0, 1, 1, 1, 2, 9])
                      for _ in range(rng.randrange(1, 9))]
            groups.append((s, submit_group(m, s, counts,
                                           rng.randrange(12, 200)), counts))
        for s, base, counts in groups:
            ok = None
            if failed:
                ok = [int(rng.random() < 0.85) for _ in counts]
            if full:
                m.group(s, 0, counts, ok=ok, n_entries=0)
            else:
                m.group(s, base, counts, ok=ok)
        for s in range(nsh):  # the failure reports, most of the time
            if m.shards[s].poisoned and rng.random() < 0.7:
                m.clear(s)
    return m


@pytest.mark.parametrize("seed", range(4))
def test_random_scenarios(driver, seed):
    """100 scenarios a seed; every kind of group must turn up."""
    rng = random.Random(7000 + seed)
    models = [random_scenario(rng) for _ in range(100)]
    keeps = [w for m in models for w in m.want if w[0] == "K"]
    assert sum(k[3] == 1 for k in keeps) > 50  # clean
    assert sum(k[3] == 0 and k[1] > 0 for k in keeps) > 20  # clean prefix
    assert sum(k == ("K", 0, 0, 0) for k in keeps) > 50  # overflow / stale
    assert any(sh.failures > 1 for m in models for sh in m.shards)
    check(driver, models)
