"""Shared by tests/test_sam_text_emu.py (the device sources on the host emulator) and tests/test_zzz_sam_text_gpu.py (the MI355X): SAM text
formatted on the device -- bm2_sam_format_dev on records made by hand against a formatter written here from the SAM field order, and the
tail with BM2_SAM_F_DEVICE_TEXT against the flag-off tail and the compiled reference."""
import numpy as np

import bm2

OPS = "MIDSH"


def contig_names(prefix):
    """names of the .ann file (bntseq.cpp:113-140: a header line, then two lines per contig)"""
    with open(prefix + ".ann") as f:
        lines = f.read().splitlines()
    n = int(lines[0].split()[1])
    return [lines[1 + 2 * i].split()[1] for i in range(n)]


def cigar_text(ops):
    return "".join("%d%s" % (l, OPS[o]) for l, o in ops) if ops else "*"


def expected_line(c, names, reads, rnames, quals, rg):
    """One SAM line from a case (a dict with the decided fields), written from the SAM field order -- not the library's host path."""
    f = [rnames[c["read"]], str(c["flag"])]
    if c["rid"] >= 0:
        f += [names[c["rid"]], str(c["pos"]), str(c["mapq"]), cigar_text(c["cigar"])]
    else:
        f += ["*", "0", "0", "*"]
    if c["mrid"] >= 0:
        f += ["=" if c["rnext_eq"] else names[c["mrid"]], str(c["mpos"]), str(c["tlen"])]
    else:
        f += ["*", "0", "0"]
    if c["no_seq"]:
        f += ["*", "*"]
    else:
        codes = reads[c["read"]][c["qb"]:c["qe"]]
        q = quals[c["read"]]
        q = None if q is None else q[c["qb"]:c["qe"]]
        if c["is_rev"]:
            f.append("".join("TGCAN"[x] for x in codes[::-1]))
            f.append("*" if q is None else q[::-1].decode())
        else:
            f.append("".join("ACGTN"[x] for x in codes))
            f.append("*" if q is None else q.decode())
    if c["cigar"]:
        f += ["NM:i:%d" % c["nm"], "MD:Z:" + c["md"].decode()]
    if c["mc"]:
        f.append("MC:Z:" + cigar_text(c["mc"]))
    if c["score"] >= 0:
        f.append("AS:i:%d" % c["score"])
    if c["sub"] >= 0:
        f.append("XS:i:%d" % c["sub"])
    if rg:
        f.append("RG:Z:" + rg.decode())
    return "\t".join(f).encode() + c["blob"] + b"\n"


def to_records(cases):
    """cases -> ([SamRec], ops, side bytes): every variable-length piece appended with its length"""
    recs, ops, side = [], [], b""
    for c in cases:
        r = bm2.SamRec()
        for k in ("read", "flag", "rid", "mapq", "pos", "mrid", "rnext_eq", "mpos", "tlen", "is_rev", "no_seq", "qb", "qe", "nm", "score", "sub"):
            setattr(r, k, c[k])
        r.cigar_off, r.n_cigar = len(ops), len(c["cigar"])
        ops += [l << 4 | o for l, o in c["cigar"]]
        r.mc_off, r.n_mc = len(ops), len(c["mc"])
        ops += [l << 4 | o for l, o in c["mc"]]
        r.md_off, r.md_len = len(side), len(c["md"])
        side += c["md"]
        r.blob_off, r.blob_len = len(side), len(c["blob"])
        side += c["blob"]
        recs.append(r)
    return recs, np.array(ops, np.uint32), side


def hand_made_cases():
    """-> (reads, read names, qualities, cases): every form a line can take (the list of the issue)"""
    rng = np.random.default_rng(77)
    reads, rnames, quals, cases = [], [], [], []

    def read(n, name, qual=True, codes=None):
        reads.append(rng.integers(0, 4, n).astype(np.uint8) if codes is None else np.array(codes, np.uint8))
        rnames.append(name)
        quals.append(bytes(rng.integers(33, 74, size=n, dtype=np.uint8)) if qual else None)
        return len(reads) - 1

    def case(rd, **kw):
        n = len(reads[rd])
        c = dict(read=rd, flag=0, rid=0, pos=101, mapq=60, cigar=[(n, 0)], mrid=-1, rnext_eq=0, mpos=0, tlen=0, is_rev=0, no_seq=0, qb=0, qe=n,
                 mc=[], nm=0, md=b"%d" % n, score=n, sub=0, blob=b"")
        c.update(kw)
        cases.append(c)

    a = read(100, "fwd")
    case(a)                                                                             # mapped forward, single-end (no mate)
    case(a, flag=16, is_rev=1, nm=2, md=b"10A80^C9", sub=-1)                            # mapped reverse
    b = read(100, "pair")
    case(b, flag=0x4 | 0x1 | 0x40 | 0x20, rid=1, pos=5000, mapq=0, cigar=[], mrid=1, rnext_eq=1, mpos=5000, is_rev=1, mc=[(100, 0)], score=-1, sub=-1)   # unmapped, borrows the mate's position
    case(b, flag=0x1 | 0x8 | 0x80, rid=1, pos=5000, mrid=1, rnext_eq=1, mpos=5000)       # its mate: the mate is unmapped
    case(a, flag=0x1 | 0x40, mrid=0, rnext_eq=1, mpos=401, tlen=400, mc=[(5, 3), (95, 0)])        # `=`, positive TLEN
    case(a, flag=0x1 | 0x80 | 0x10, is_rev=1, pos=401, mrid=0, rnext_eq=1, mpos=101, tlen=-400, mc=[(100, 0)])   # negative TLEN
    case(a, flag=0x1 | 0x40, mrid=2, rnext_eq=0, mpos=77, tlen=0, mc=[(100, 0)])                  # named RNEXT, TLEN 0
    case(a, pos=1, flag=0x1 | 0x40, mrid=0, rnext_eq=1, mpos=9999999999, tlen=9999999998, mc=[(100, 0)])     # POS of one digit, PNEXT of ten
    case(a, pos=9999999999, flag=0x1 | 0x40, mrid=0, rnext_eq=1, mpos=1, tlen=-9999999998, mc=[(100, 0)])    # and the other way round
    case(a, flag=0x800, cigar=[(30, 4), (70, 0)], qb=30, qe=100, md=b"70", blob=b"\tSA:Z:chrA,5,+,30M70S,60,0;")       # supplementary, hard clip, forward
    case(a, flag=0x800 | 0x10, is_rev=1, cigar=[(60, 0), (40, 4)], qb=40, qe=100, md=b"60")                           # ... reverse: SEQ / QUAL shortened at the right end
    case(a, flag=0x800, cigar=[(70, 0), (30, 4)], qb=0, qe=70, md=b"70")
    case(a, flag=0x100, no_seq=1, sub=-1)                                                # secondary: `*\t*`
    nq = read(50, "noqual", qual=False)
    case(nq)                                                                            # no qualities
    case(nq, flag=16, is_rev=1)
    one = read(1, "one")
    case(one)                                                                           # a read of length 1
    case(one, flag=16, is_rev=1)
    nn = read(12, "enns", codes=[0, 4, 1, 4, 4, 2, 3, 4, 0, 1, 2, 3])
    case(nn)                                                                            # N bases
    case(nn, flag=16, is_rev=1)
    long_cg = read(200, "ops40")
    ops40 = [(3 + (k % 3), 0) if k % 2 == 0 else (1 + k % 2, 1 + (k // 2) % 2) for k in range(40)]
    ops40[-1] = (200, 0)
    case(long_cg, cigar=ops40, mc=ops40[:7], mrid=0, rnext_eq=1, mpos=3, tlen=-5, flag=0x1 | 0x40, nm=39, md=b"3^AC4T0")      # a CIGAR of 40 ops (and 1 above)
    case(a, blob=b"\tXA:Z:chrB,-100,100M,1;\tco:Z:a comment")                            # a non-empty blob
    for k in range(1, 34):                                                              # names of every length: lines start at every residue modulo 16
        case(read(30 + k, "n" * k), pos=10 ** (k % 9), flag=16 * (k & 1), is_rev=k & 1)
    big = read(40000, "forty_kb")
    case(big, cigar=[(12345, 0), (5, 1), (27650, 0)], md=b"40000", nm=5)                 # longer than any LDS window
    case(big, flag=16, is_rev=1, cigar=[(40000, 0)], md=b"40000")
    case(a)
    return reads, rnames, quals, cases


def check_hand_made_records(ctx, prefix):
    """bm2_sam_format_dev against expected_line; the cap rule; the counters.  Fails on a library without the entry point."""
    names = contig_names(prefix)
    assert len(names) >= 3, names
    reads, rnames, quals, cases = hand_made_cases()
    enc = np.concatenate(reads).astype(np.uint8)
    ln = np.array([len(r) for r in reads], np.int32)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
    recs, ops, side = to_records(cases)
    for rg in (None, b"grp1"):
        so = bm2.default_sam_opt(rg_id=rg)
        exp = b"".join(expected_line(c, names, reads, rnames, quals, rg) for c in cases)
        got = ctx.sam_format(so, enc, off, ln, rnames, recs, ops, side, quals=quals)
        if got != exp:
            la, lb = exp.splitlines(), got.splitlines()
            for i, (x, y) in enumerate(zip(la, lb)):
                assert x == y, "rg %r record %d\n  expected %r\n  got      %r" % (rg, i, x[:300], y[:300])
            assert len(la) == len(lb), (len(la), len(lb))
            assert False, "texts differ in their line ends"
        n_rec, dev, host = bm2.sam_text_stats()
        assert n_rec == len(cases) and dev + host == len(exp) and host == sum(len(c["blob"]) for c in cases), (n_rec, dev, host, len(exp))
        starts = np.cumsum([0] + [len(expected_line(c, names, reads, rnames, quals, rg)) for c in cases])[:-1]
        assert set(int(s) % 16 for s in starts) == set(range(16))           # every head / tail alignment of a line inside a tile
    # one byte short: BM2_ECAP, the exact size, nothing written
    so = bm2.default_sam_opt()
    exp = b"".join(expected_line(c, names, reads, rnames, quals, None) for c in cases)
    guard = np.full(len(exp) + 32, 0xA5, np.uint8)
    try:
        ctx.sam_format(so, enc, off, ln, rnames, recs, ops, side, quals=quals, out=guard[16:16 + len(exp) - 1])
        assert False, "a capacity one byte short was accepted"
    except bm2.Bm2Error as e:
        assert e.rc == bm2.BM2_ECAP and e.need == len(exp), (e.rc, e.need, len(exp))
    assert (guard == 0xA5).all()
    got = ctx.sam_format(so, enc, off, ln, rnames, recs, ops, side, quals=quals, out=guard[16:16 + len(exp)])
    assert got == exp and (guard[:16] == 0xA5).all() and (guard[16 + len(exp):] == 0xA5).all()
    # an empty batch
    assert ctx.sam_format(so, enc, off, ln, rnames, [], (), b"", quals=quals) == b"" and bm2.sam_text_stats() == (0, 0, 0)
    # a record that points outside its arrays is refused before any kernel runs
    bad = bm2.SamRec.from_buffer_copy(bytes(recs[0]))
    bad.cigar_off = len(ops)
    try:
        ctx.sam_format(so, enc, off, ln, rnames, [bad], ops, side, quals=quals)
        assert False, "a record pointing outside the ops was accepted"
    except bm2.Bm2Error as e:
        assert e.rc == bm2.BM2_EINVAL
    return len(cases), len(exp)


def check_text_stats(text, blob_cap=None):
    """after a tail call with the bit: the counters describe this text; blob_cap: the share of pre-formatted bytes allowed"""
    n_rec, dev, host = bm2.sam_text_stats()
    assert n_rec == text.count(b"\n") and dev + host == len(text), (n_rec, dev, host, len(text), text.count(b"\n"))
    if blob_cap is not None:
        assert host <= blob_cap * (dev + host), (host, dev)
    return n_rec, dev, host


def tail_se(M, fa, reads, names, quals, ref, ctx, okw=None, flag=0, Tmin=30, comments=None, rg=None, n_threads=0, blob_cap=None):
    """M = the test_sam_tail module.  bm2_sam_se_dev with the bit == without == the reference's text"""
    kw = dict(flag=flag, T=Tmin, n_threads=n_threads)
    if rg:
        kw["rg_id"] = rg
    off_text = M._ours(fa, reads, names, quals, okw, bm2.default_sam_opt(**kw), comments=comments, ctx=ctx)
    kw["flag"] = flag | bm2.SAM_F_DEVICE_TEXT
    on_text = M._ours(fa, reads, names, quals, okw, bm2.default_sam_opt(**kw), comments=comments, ctx=ctx)
    assert ref == off_text, M._diff(ref, off_text)
    assert ref == on_text, M._diff(ref, on_text)
    return check_text_stats(on_text, blob_cap)


def tail_pe(M, d, fa, r1, r2, extra, ctx, flag=0, okw=None, blob_cap=None, **skw):
    """bm2_sam_pe_dev with the bit == without == the reference's text; the rescue / CIGAR counters do not move"""
    ref, off_text, _ = M._pe_run(d, fa, r1, r2, extra, flag=flag, okw=okw, ctx=ctx, **skw)
    st_off = (bm2.sam_rescue_stats(), bm2.sam_cigar_stats())
    ref2, on_text, _ = M._pe_run(d, fa, r1, r2, extra, flag=flag | bm2.SAM_F_DEVICE_TEXT, okw=okw, ctx=ctx, **skw)
    assert (bm2.sam_rescue_stats(), bm2.sam_cigar_stats()) == st_off, (st_off, bm2.sam_rescue_stats(), bm2.sam_cigar_stats())
    assert ref == off_text, M._diff(ref, off_text)
    assert ref == on_text, M._diff(ref, on_text)
    check_text_stats(on_text, blob_cap)
    return ref
