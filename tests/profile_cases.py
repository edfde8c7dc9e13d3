"""A plain model of the sequence profile (include/mtg_fill.h: mtg_index_profile_sequences), to judge the device's words and runs.

Given the solid canonical k-mers with their counts and a list of strings it gives, per position, the expected word (abundance, successor and
predecessor mask, valid, present) and the maximal runs of valid, absent positions with their flags.  It knows nothing of the product: k-mers are
looked up in a Python dict, neighbours by eight look-ups, runs by a loop over positions.  Strings hold ACGTNacgtn only (N / n is the invalid
character, lower case counts as upper case)."""
import numpy as np

from tests.reads_cases import CODE, canon, kmask, plain_count

RUN_DTYPE = np.dtype([("seq", np.uint32), ("start", np.uint32), ("length", np.uint32), ("flags", np.uint32)])


def solid_of_files(files, k, lo):
    """{canonical k-mer: min(count, 255)} of the k-mers seen at least lo times in the files"""
    return {c: min(n, 255) for c, n in plain_count(files, k).items() if n >= lo}


def words_of(solid, k, seq):
    """the expected uint32 word of every position of seq"""
    n = max(len(seq) - k + 1, 0)
    out = np.zeros(n, np.uint32)
    up = seq.upper()
    mk = kmask(k)
    for p in range(n):
        w = up[p:p + k]
        if "N" in w:
            continue
        x = 0
        for ch in w:
            x = (x << 2) | CODE[ch]
        word = 1 << 16
        a = solid.get(canon(x, k), 0)
        if a:
            succ = sum(1 << nt for nt in range(4) if canon(((x << 2) | nt) & mk, k) in solid)
            pred = sum(1 << nt for nt in range(4) if canon((x >> 2) | (nt << (2 * (k - 1))), k) in solid)
            word |= (1 << 17) | a | (succ << 8) | (pred << 12)
        out[p] = word
    return out


def runs_of_words(words_per_seq):
    """the runs of a list of per-sequence word arrays: the literal loop over positions"""
    runs = []
    for s, ws in enumerate(words_per_seq):
        valid = [(int(w) >> 16) & 1 for w in ws]
        present = [(int(w) >> 17) & 1 for w in ws]
        p, n = 0, len(ws)
        while p < n:
            if not (valid[p] and not present[p]):
                p += 1
                continue
            e = p
            while e < n and valid[e] and not present[e]:
                e += 1
            flags = (1 if p > 0 and present[p - 1] else 0) | (2 if e < n and present[e] else 0)
            runs.append((s, p, e - p, flags))
            p = e
    return np.array(runs, dtype=RUN_DTYPE) if runs else np.zeros(0, RUN_DTYPE)


def profile(solid, k, seqs):
    """(list of word arrays, runs) expected for seqs"""
    words = [words_of(solid, k, s) for s in seqs]
    return words, runs_of_words(words)


def read_fasta(path):
    """[(name up to the first blank, sequence)] of a FASTA file, lines joined"""
    recs = []
    for line in open(path).read().splitlines():
        if line.startswith(">"):
            recs.append([line[1:].split()[0] if line[1:].split() else "", []])
        elif recs:
            recs[-1][1].append(line.strip())
    return [(n, "".join(p)) for n, p in recs]


def gold_hom_records(path):
    """[(sequence name, pos, fuzzy, left_kmer)] of the HOM records of a .breakpoints file"""
    out = []
    lines = open(path).read().splitlines()
    for i, l in enumerate(lines):
        if l.startswith(">") and l.split()[0].endswith("_HOM") and l.split()[-1] == "left_kmer":
            f = l[1:].split()[0].split("_")
            out.append((f[1], int(f[3]), int(f[5]), lines[i + 1].strip()))
    return out
