"""The whole fill at k below 31 and with off-default limits, against the oracle: shared by the emulator suite (tests/test_kfill_cpu.py) and the GPU
suite (tests/test_gpu_kfill.py).  Every function takes the module to test (mindthegap_amd, or the product on the emulator), k and parameters.
Everything is bit-exact (integers, bytes, text).  Every case asserts ON THE ORACLE'S OUTPUT ALONE that it exercised what it claims: a floor on the
filled sites, limits that bind, a fill count that rises with nb_mis_allowed, the targets per seed."""
import re
import struct

import numpy as np
import pytest

from mindthegap_amd.synth import SynthSet
from tests import oracle_lib, text_cases


def _read(p):
    with open(p) as f:
        return f.read()


def _vcf_body(p):
    return [l for l in _read(p).splitlines() if not l.startswith("##")]


def write_idx(path, km, ct, k, amin=3):
    """an MTGIDX1 container of the oracle's k-mers"""
    with open(path, "wb") as f:
        f.write(b"MTGIDX1\0" + struct.pack("<4i", k, amin, -1, 0) + struct.pack("<Q", len(km)) + km.tobytes() + ct.astype(np.uint32).tobytes())


def sub(t, i):
    return t[:i] + ("A" if t[i] not in "Aa" else "C") + t[i + 1:]


def records(path):
    """{site: [(sequence, qual)]} of an .insertions.fasta file; the site is the header up to its _len_ field"""
    out, key, qual = {}, None, None
    for l in _read(path).splitlines():
        if l.startswith(">"):
            key = l[1:].split("_len_")[0]
            qual = int(re.search(r"_qual_(\d+)_", l).group(1))
        elif key is not None:
            out.setdefault(key, []).append((l, qual))
    return out


def compare_bkpt_files(hip, cpu, extend=False):
    for ext in [".insertions.fasta", ".info.txt"] + ([".extensions.fasta"] if extend else []):
        assert _read(hip + ext) == _read(cpu + ext), ext
    assert _vcf_body(hip + ".insertions.vcf") == _vcf_body(cpu + ".insertions.vcf")


# ---- case 1: the bkpt sweep ------------------------------------------------------------------------------------------------------------------
BKPT_KS = (31, 27, 24, 23, 21, 16, 13)  # 31: the control; 24 / 23: the piece index usable / not usable at nb_mis = 2
# -max-nodes / -max-length that bind for the set of (k, het_snps): chosen from the oracle's output alone (bkpt_sweep asserts that they bind there).
# At k >= 21 the forks of bkpt_set are all that branches (five or six sites of the 60 lose their fill under 3 / 100); at k = 16 and 13 chance repeats of
# k - 1 nucleotides branch too (5 / 150: seven and 19 sites differ).
BKPT_LIMITS = {(k, het): (3, 100) if k >= 21 else (5, 150) for k in BKPT_KS for het in (0, 2)}
# the oracle's own count of filled sites (of 60) with -extend, per (k, het_snps): the floor of each set.  A fifth of the sites cannot be filled (three
# substitutions, a substitution under REPEATED); at k = 13 the chance repeats leave 26.
BKPT_FLOOR = {(k, het): 48 if k >= 16 else 26 for k in BKPT_KS for het in (0, 2)}
BKPT_SEED = 44


def bkpt_set(k, het):
    """60 sites on 60 sequences (haploid) or on 60 loci of two haplotypes that differ by two SNPs each; returns (set, sequences of the index).
    A walk over such a set is one node, which no limit can bind.  So every third site with an insertion of 120 nt or more gets a fork in the middle
    of its insertion: one more sequence of the index, 2 k nucleotides of the donor followed by 150 unrelated ones.  The fill of such a site is a
    gap of several contigs, with its target behind the fork."""
    S = SynthSet(nseq=120 if het else 60, n_sites=60, seed=BKPT_SEED, k=k, het_snps=het)
    seqs = [S.ascii(j) for j in range(S.nseq)]
    rng = np.random.default_rng(1000 + k)
    for i in range(0, S.n_sites, 3):
        p, L = int(S.pos[i]), int(S.ins_len[i])
        if L < 120:
            continue
        q = p + L // 2
        tail = "".join("ACGT"[c] for c in rng.integers(0, 4, 150))
        seqs.append(seqs[i][q - 2 * k:q] + sub(seqs[i][q], 0) + tail)
    return S, seqs


def pack_sequences(seqs):
    """(words, word offsets, lengths) of ASCII sequences as 2-bit codes, 32 per word, every sequence from a word of its own (SynthSet.packed's layout)"""
    code = np.zeros(256, dtype=np.uint64)
    for c, v in zip(b"ACTG", range(4)):
        code[c] = v
    sh = np.arange(32, dtype=np.uint64) * np.uint64(2)
    words, off, n = [], [], 0
    for s in seqs:
        c = np.zeros((len(s) + 31) // 32 * 32 + 32, dtype=np.uint64)
        c[:len(s)] = code[np.frombuffer(s.encode(), dtype=np.uint8)]
        w = (c.reshape(-1, 32) << sh[None, :]).sum(axis=1, dtype=np.uint64)
        off.append(n)
        n += len(w)
        words.append(w)
    return np.concatenate(words), np.array(off, dtype=np.uint64), np.array([len(s) for s in seqs], dtype=np.uint32)


def write_broken_breakpoints(S, path):
    """the anchors broken by position as a function of k, one kind per site number modulo 10"""
    k = S.k
    with open(path, "w") as f:
        for i in range(S.n_sites):
            l, r, _ = S.site(i)
            tag, v = "", i % 10
            if v == 1: l = sub(l, k // 2)                               # left anchor in the middle: the forward attempt fails, the reverse one fills
            elif v == 2: r = sub(r, 0)                                  # one substitution, the first nucleotide
            elif v == 3: r = sub(sub(r, 0), k - 1)                      # two: the first and the last nucleotide, the middle piece is intact
            elif v == 4: r = sub(sub(r, k // 2 - 1), k // 2)            # two inside one piece (the middle one of three)
            elif v == 5: r = sub(sub(sub(r, 0), k // 2), k - 1)         # three: one in every piece, not found with nb_mis = 2
            elif v == 6: r = r[:k // 3] + "N" + r[k // 3 + 1:]          # an N: one forced mismatch
            elif v == 7: r = r.lower()
            elif v == 8: r, tag = sub(r, k // 2), " REPEATED"           # repeated anchors allow no mismatch
            elif v == 9: tag = " REPEATED"
            f.write(">%s%s left_kmer\n%s\n>%s%s right_kmer\n%s\n" % (S.site_name(i), tag, l, S.site_name(i), tag, r))


def _sites_that_differ(a, b):
    ra, rb = records(a), records(b)
    return sum(1 for s in set(ra) | set(rb) if ra.get(s) != rb.get(s))


def bkpt_sweep(mtg, tmp_path, k, het, index_file=None, oracle=None):
    """the tool against oracle.fill_files on the broken anchors: with -extend, with -fwd-only -filter, and with -max-nodes / -max-length that bind.
    index_file / oracle: a container and the oracle index of the same set from another source (the GPU suite's packed-built index)."""
    S, seqs = bkpt_set(k, het)
    o = oracle or oracle_lib.Index.from_sequences(seqs, k, 3, 40)
    idxf = index_file
    if idxf is None:
        idxf = str(tmp_path / "s.mtgidx")
        km, ct = o.export()
        write_idx(idxf, km, ct, k)
    bk = str(tmp_path / "s.breakpoints")
    write_broken_breakpoints(S, bk)
    nodes, length = BKPT_LIMITS[(k, het)]
    for tag, extra, okw in (("a", ["-extend"], dict(extend=1)), ("b", ["-fwd-only", "-filter"], dict(fwd_only=1, filter=1)),
                            ("c", ["-max-nodes", str(nodes), "-max-length", str(length)], dict(max_nodes=nodes, max_depth=length))):
        cpu, hip = str(tmp_path / ("cpu" + tag)), str(tmp_path / ("hip" + tag))
        o.fill_files("bkpt", bk, cpu, params=oracle_lib.default_params(**okw))
        assert mtg.Filler().run(["-graph", idxf, "-bkpt", bk, "-out", hip] + extra) == 0
        compare_bkpt_files(hip, cpu, extend="-extend" in extra)
    # what the case claims, on the oracle's files alone
    ra = records(str(tmp_path / "cpua.insertions.fasta"))
    assert len(ra) >= BKPT_FLOOR[(k, het)], len(ra)
    quals = {q for v in ra.values() for _, q in v}
    assert {50, 25, 10, 5} <= quals, quals  # exact, repeated, one and two differences in the anchor
    assert _sites_that_differ(str(tmp_path / "cpua.insertions.fasta"), str(tmp_path / "cpuc.insertions.fasta")) >= 5  # the limits bind
    assert len(records(str(tmp_path / "cpub.insertions.fasta"))) < len(ra)  # the reverse attempts are gone
    if oracle is None:
        o.close()


# ---- case 2: short fills at every alignment ---------------------------------------------------------------------------------------------------
SHORT_KS = (24, 21, 16)
SHORT_FLOOR = {24: 140, 21: 140, 16: 140}  # the oracle's count of filled sites (of 140) per k


def short_fills(mtg, tmp_path, k):
    """fills of 1 .. 70 nucleotides, a third by the reverse attempt: the lean forms' 8-byte abundance reads and 16-byte ASCII pieces, with a k-mer
    count per fill that changes with k.  The caller sets MTG_HOST_FORMAT for the host's writers."""
    S = SynthSet(nseq=160, n_sites=140, seed=23, ins_min=1, ins_max=70, k=k)
    o = oracle_lib.Index.from_sequences([S.ascii(j) for j in range(S.nseq)], k, 3, 40)
    km, ct = o.export()
    bk = str(tmp_path / "short.breakpoints")
    with open(bk, "w") as f:
        for i in range(S.n_sites):
            l, r, _ = S.site(i)
            if i % 3 == 1:
                l = sub(l, k // 2)
            f.write(">%s left_kmer\n%s\n>%s right_kmer\n%s\n" % (S.site_name(i), l, S.site_name(i), r))
    idxf = str(tmp_path / "short.mtgidx")
    write_idx(idxf, km, ct, k)
    cpu, hip = str(tmp_path / "cpu"), str(tmp_path / "hip")
    o.fill_files("bkpt", bk, cpu)
    assert mtg.Filler().run(["-graph", idxf, "-bkpt", bk, "-out", hip]) == 0
    compare_bkpt_files(hip, cpu)
    rc = records(cpu + ".insertions.fasta")
    assert len(rc) >= SHORT_FLOOR[k], len(rc)
    assert len({len(s) % 8 for v in rc.values() for s, _ in v}) == 8  # every alignment of the 8-byte words
    o.close()


# ---- case 3: nb_mis_allowed ------------------------------------------------------------------------------------------------------------------
MIS_KS = (31, 24, 23, 17, 13)
MIS_FILLED = {31: [10, 20, 30, 40, 50], 24: [10, 20, 30, 40, 50], 23: [10, 20, 30, 40, 50], 17: [10, 20, 30, 40, 50], 13: [6, 11, 19, 35, 47]}  # the oracle's count of filled sites (of 50) for nb_mis_allowed = 0 .. 4, per k


def _spread(k, m):
    """m positions from the first to the last nucleotide"""
    return [0] if m == 1 else [round(j * (k - 1) / (m - 1)) for j in range(m)]


def nb_mis_case(mtg, tmp_path, k):
    """nb_mis_allowed 0 .. 4 through fill_batch and through a prepared batch; the target of site i carries i % 5 substitutions"""
    from mindthegap_amd import lib as L
    S = SynthSet(nseq=60, n_sites=50, seed=43, k=k)
    o = oracle_lib.Index.from_sequences([S.ascii(j) for j in range(S.nseq)], k, 3, 40)
    km, ct = o.export()
    idx = mtg.Index.from_kmers(km, ct, k)
    gaps, names = [], []
    bk = str(tmp_path / "mis.breakpoints")
    with open(bk, "w") as f:
        for i in range(S.n_sites):
            l, r, _ = S.site(i)
            for p in (_spread(k, i % 5) if i % 5 else []):
                r = sub(r, p)
            names.append(S.site_name(i))
            gaps.append(mtg.Gap(l, r, [(r, S.site_name(i), False)]))
            f.write(">%s left_kmer\n%s\n>%s right_kmer\n%s\n" % (S.site_name(i), l, S.site_name(i), r))
    counts = []
    batches = {}
    for n in range(5):
        cpu = str(tmp_path / ("cpu%d" % n))
        o.fill_files("bkpt", bk, cpu, params=oracle_lib.default_params(nb_mis_allowed=n, fwd_only=1))
        want = records(cpu + ".insertions.fasta")
        counts.append(len(want))
        want = [want.get(name, []) for name in names]
        params = mtg.FillParams(nb_mis_allowed=n)
        got = idx.fill_batch(gaps, params)
        assert [[(f["seq"], f["qual"]) for f in r["filled"]] for r in got] == want, n
        batches[n] = idx.prepare_batch(gaps, params)
        h, nf, _ = idx.fill_prepared(batches[n], params)
        try:
            got = L._results_dicts(idx.lib, h, len(gaps))
        finally:
            idx.free_results(h)
        assert [[(f["seq"], f["qual"]) for f in r["filled"]] for r in got] == want, n
        assert nf.tolist() == [len(w) for w in want]
    assert counts == MIS_FILLED[k] and all(a < b for a, b in zip(counts, counts[1:])), counts  # (the oracle's) rises with nb_mis_allowed
    # a batch marshalled for one allowance is refused with another
    for n, other in ((2, 1), (0, 3), (4, 2)):
        with pytest.raises(L.MtgError) as e:
            idx.fill_prepared(batches[n], mtg.FillParams(nb_mis_allowed=other))
        assert e.value.code == 2  # MTG_ERR_ARG
    for b in batches.values():
        b.close()
    idx.close()
    o.close()


# ---- case 4: contig mode with at least 16 targets per seed -------------------------------------------------------------------------------------
CONTIG_KS = (31, 24, 23, 21, 16)  # 24 / 23: the piece index on / off
CONTIG_OVERLAPS = (0, 5, 10, "k+5")  # the tool raises an overlap below k to k: the fourth value is one that it takes as given
CONTIG_FLOOR = 14  # the oracle's count of filled holes (GFA segments with a fill), the same for every k and overlap of these sets


def contig_files(tmp_path, k):
    """12 donor sequences cut into 24 contigs around their holes; the right contigs' target k-mers (contig[k:2k]) differ from the graph -- one, two or
    three substitutions, an N, lower case -- as in the many-targets case of the emulator suite, at positions that are expressions of k"""
    S = SynthSet(nseq=12, n_sites=12, seed=31, k=k)
    seqs = [S.ascii(j) for j in range(S.nseq)]
    o = oracle_lib.Index.from_sequences(seqs, k, 3, 40)
    km, ct = o.export()
    contigs = str(tmp_path / "contigs.fa")
    with open(contigs, "w") as f:
        for j, s in enumerate(seqs):
            p, L = int(S.pos[j]), int(S.ins_len[j])
            right = s[p + L:]
            m = j % 8
            if m == 1: right = sub(right, k + k // 6)
            elif m == 2: right = sub(sub(right, k), 2 * k - 1)                          # the first and the last nucleotide of the target
            elif m == 3: right = sub(sub(sub(right, k + 2), k + k // 2), 2 * k - 3)     # three: not found
            elif m == 4: right = right[:k + k // 3] + "N" + right[k + k // 3 + 1:]      # one forced mismatch
            elif m == 5: right = right[:k] + right[k:2 * k].lower() + right[2 * k:]
            elif m == 6: right = sub(sub(right, k + k // 2 - 1), k + k // 2)            # both in one piece
            f.write(">c%dL\n%s\n>c%dR\n%s\n" % (j, s[:p], j, right))
    idxf = str(tmp_path / "c.mtgidx")
    write_idx(idxf, km, ct, k)
    return o, idxf, contigs


CONTIG_EXTS = ("_seed_dictionary.fasta", ".info.txt", ".gfa", ".insertions.fasta")


def contig_case(mtg, tmp_path, k, monkeypatch, per_seed_too):
    """the tool in contig mode against the oracle, -overlap 0 / 5 / 10, files as sorted lines (the oracle's records come in completion order).
    per_seed_too: also with CONTIG_PER_SEED=1 (a dictionary per seed instead of the shared target table); the two products' files must be identical."""
    o, idxf, contigs = contig_files(tmp_path, k)
    for ov in [k + 5 if v == "k+5" else v for v in CONTIG_OVERLAPS]:
        cpu = str(tmp_path / ("cpu%d" % ov))
        o.fill_files("contig", contigs, cpu, params=oracle_lib.default_params(nb_cores=4, overlap=ov))
        # the oracle's own files: every seed's dictionary holds the other contigs' ends, 16 at least (POST_INDEX_MIN), and holes are filled
        n_seeds = _read(cpu + "_seed_dictionary.fasta").count(">")
        assert n_seeds - 2 >= 16, n_seeds
        nfill = sum(1 for l in _read(cpu + ".gfa").splitlines() if l.startswith("S") and ";" in l)
        assert nfill >= CONTIG_FLOOR, nfill
        runs = [("hip%d" % ov, None)] + ([("seed%d" % ov, "1")] if per_seed_too else [])
        for name, per_seed in runs:
            if per_seed:
                monkeypatch.setenv("MTG_CONTIG_PER_SEED", per_seed)
            else:
                monkeypatch.delenv("MTG_CONTIG_PER_SEED", raising=False)
            hip = str(tmp_path / name)
            assert mtg.Filler().run(["-graph", idxf, "-contig", contigs, "-overlap", str(ov), "-out", hip]) == 0
            for ext in CONTIG_EXTS:
                assert sorted(_read(hip + ext).splitlines()) == sorted(_read(cpu + ext).splitlines()), (ov, name, ext)
        monkeypatch.delenv("MTG_CONTIG_PER_SEED", raising=False)
        if per_seed_too:
            for ext in CONTIG_EXTS:
                assert _read(str(tmp_path / ("hip%d" % ov)) + ext) == _read(str(tmp_path / ("seed%d" % ov)) + ext), (ov, ext)
    o.close()


# ---- case 5: the text entry ------------------------------------------------------------------------------------------------------------------
TEXT_KS = (24, 21, 16, 13)


def text_case(mtg, tmp_path, k):
    """mtg_fill_text (block copied, block registered) against the string entry at k, and both against the oracle's sequences for the plain sites"""
    seen = []

    def check(S, o, gaps, res):
        plain = [i for i in range(S.n_sites) if i % 10 == 9]
        bk = str(tmp_path / ("plain%d.breakpoints" % len(seen)))
        S.write_breakpoints(bk, plain)
        cpu = str(tmp_path / ("cpu%d" % len(seen)))
        o.fill_files("bkpt", bk, cpu, params=oracle_lib.default_params(fwd_only=1))
        want = records(cpu + ".insertions.fasta")
        assert len(want) >= 2, len(want)  # (k = 13: chance repeats leave two of the four)
        for i in plain:
            assert [(f["seq"], f["qual"]) for f in res[i]["filled"]] == want.get(S.site_name(i), []), i
        # a key shorter than k (site 4 of every ten) can never be matched (mtg_post.h: encode_target), an empty dictionary (site 5) neither: both
        # entries agree on these sites, and no oracle run can say so -- the reference reads such a key past its end
        for i in range(S.n_sites):
            if i % 10 in (4, 5):
                assert res[i]["nb_terminal"] == 0 and res[i]["filled"] == [], i
        seen.append(len(want))

    text_cases.run(mtg, oracle_lib, k, check)
    assert len(seen) == 2
