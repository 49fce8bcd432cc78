"""The catalog of LZ4 frames with linked blocks (achip_ctx_set_lz4frame_linked_blocks): every case is an item for the LZ4 frame reader, built by the writers of
tests/lz4_linked_ref.py so that it holds ONE named edge -- of the rule itself (where a match's source may lie), of the output ring of the reader's block decoder
(OUT_RING = 4096, LDS_REACH = 3056 bytes served from LDS), or of the frame's structure around linked blocks.

    cases()            [Case]; built once
    Case               name, label (the edge it stands for), data (the item), cap (output capacity), linked (the item holds a frame of linked blocks),
                       plain (what it decodes to with the setting on; None: it fails), status / offset (of that failure), claims (what the bytes must show for
                       the label to be true)
    claim_failures(c)  the claims of a case that its bytes do not bear out, from lz4_linked_ref.walk(c.data) -- a reading of the item that knows nothing of how
                       it was built

With the setting off every case with `linked` fails with ACHIP_D_LZ4F_LINKED_BLOCKS at linked_descriptor(c); every other case is the Java reader's business
either way (the oracle answers for it)."""
import collections

from tests import common
from tests import lz4_linked_ref as ref

OUT_RING, LDS_REACH = 4096, 3056  # lz4_frame.hip: Rings<64, 2048, 4096, 1>
Case = collections.namedtuple("Case", "name label data cap linked plain status offset claims")

OFFSET_OUTSIDE = ref.malformed(ref.D_LZ4_OFFSET_OUTSIDE)


def lit(n):
    """a compressed block that is one literal run"""
    return ("seqs", [], n)


def one(literals, ml, offset, tail=12):
    """a compressed block of one sequence and its final literals"""
    return ("seqs", [(literals, ml, offset)], tail)


def text(n, seed=20261021):
    """n bytes of the shared generator's word soup (tests/common.py: synthetic_blocks, kind 1)"""
    data = common.synthetic_blocks(seed, 2, block_size=n)[1]
    assert len(data) == n
    return data


def linked_descriptor(case):
    """the position of the FLG byte of the item's first frame of linked blocks: where the reader without the setting stops"""
    return next(f.at + 4 for f in ref.walk(case.data) if f.linked)


def _seq_facts(frames, f, b, s):
    block = frames[f].blocks[b]
    q = block.seqs[s]
    return {"pos": q.pos, "offset": q.offset, "ml": q.ml, "source": q.pos - q.offset, "source_end": q.pos - q.offset + q.ml, "history": block.start, "ip": q.ip,
            "reach": q.pos + min(block.start, ref.MAX_DISTANCE)}


def claim_failures(case):
    frames = ref.walk(case.data)
    bad = []
    for claim in case.claims:
        kind = claim[0]
        if kind == "seq":  # ("seq", frame, block, sequence, {fact: value})
            facts = _seq_facts(frames, *claim[1:4])
            bad += ["%r: %s is %r" % (claim, k, facts[k]) for k, v in claim[4].items() if facts[k] != v]
        elif kind == "block":  # ("block", frame, block, {field: value})
            block = frames[claim[1]].blocks[claim[2]]
            bad += ["%r: %s is %r" % (claim, k, getattr(block, k)) for k, v in claim[3].items() if getattr(block, k) != v]
        elif kind == "flag":  # ("flag", frame, FLG bit, set)
            if bool(frames[claim[1]].flg & claim[2]) != claim[3]:
                bad.append("%r: FLG is %#x" % (claim, frames[claim[1]].flg))
        elif kind == "frames":  # ("frames", [linked, ...]): the item's frames in order
            if [f.linked for f in frames] != claim[1]:
                bad.append("%r: %r" % (claim, [f.linked for f in frames]))
        elif kind == "blocks":  # ("blocks", frame, count, block_max)
            if len(frames[claim[1]].blocks) != claim[2] or frames[claim[1]].block_max != claim[3]:
                bad.append("%r: %d blocks of at most %d" % (claim, len(frames[claim[1]].blocks), frames[claim[1]].block_max))
        elif kind == "cross":  # ("cross", frame, at least this many sequences per later block whose source begins in front of their block)
            for k, block in enumerate(frames[claim[1]].blocks[1:], 1):
                n = sum(1 for q in block.seqs if q.offset > q.pos)
                if n < claim[2]:
                    bad.append("%r: block %d has %d" % (claim, k, n))
        elif kind == "contained":  # ("contained", frame): no sequence's source begins in front of its block
            if any(q.offset > q.pos for block in frames[claim[1]].blocks for q in block.seqs):
                bad.append("%r" % (claim,))
        elif kind == "skippable":  # ("skippable", position)
            if int.from_bytes(case.data[claim[1]:claim[1] + 4], "little") & ref.SKIPPABLE_MASK != ref.SKIPPABLE_MAGIC:
                bad.append("%r" % (claim,))
        elif kind == "cap":  # ("cap", content bytes missing)
            if sum(f.content for f in frames) - case.cap != claim[1]:
                bad.append("%r: content %d, capacity %d" % (claim, sum(f.content for f in frames), case.cap))
        else:
            raise AssertionError(claim)
    return bad


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = _build()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def _build():
    out = []
    salt = [0]

    def content(data):
        return sum(f.content for f in ref.walk(data))

    def add(name, label, data, plain, claims, status=0, offset=0, cap=None, linked=True):
        if cap is None:
            cap = len(plain) if plain is not None else content(data) + 64
        out.append(Case(name, label, bytes(data), cap, linked, plain if status == 0 else None, status, offset, claims))

    def fr(blocks, **kw):
        salt[0] += 1
        return ref.frame(blocks, salt=salt[0], **kw)

    def valid(name, label, blocks, claims, **kw):
        f = fr(blocks, **kw)
        assert f.plain is not None, name
        add(name, label, f.data, f.plain, [("frames", [True])] + claims)

    # ---- where the source of a match may lie ----
    valid("offset 1 at a block's first byte", "a two-block frame whose second block opens with a match at offset 1",
          [lit(50), one(0, 20, 1)], [("blocks", 0, 2, 65536), ("seq", 0, 1, 0, {"pos": 0, "offset": 1, "source": -1})])
    valid("offset equals the history", "the offset is exactly the bytes of this frame produced so far",
          [lit(300), one(5, 8, 305)], [("seq", 0, 1, 0, {"pos": 5, "history": 300, "offset": 305, "reach": 305, "source": -300})])
    f = fr([lit(300), one(5, 8, 306)])
    assert f.plain is None
    add("offset is the history plus one", "one byte more than this frame has produced: offset outside destination buffer, at the block decoder's offset",
        f.data, None, [("frames", [True]), ("seq", 0, 1, 0, {"pos": 5, "history": 300, "offset": 306, "reach": 305, "ip": 8})], OFFSET_OUTSIDE, 8)
    valid("offset 65535", "the format's largest distance, with 65 536 bytes of history in front of the block (256 KiB blocks: a literal run of 64 KiB is longer than 64 KiB)",
          [lit(65536), one(0, 30, 65535)], [("seq", 0, 1, 0, {"pos": 0, "history": 65536, "offset": 65535, "reach": 65535})], size_id=5)
    valid("offset 65535 behind two blocks", "more history than a match can reach: 65 536 + 100 bytes, the source in the first block",
          [lit(65536), lit(100), one(7, 9, 65535)], [("seq", 0, 2, 0, {"pos": 7, "history": 65636, "offset": 65535, "source": -65528})], size_id=5)
    valid("straddling periodic match", "offset 3, length 40 at block position 1: the source begins two bytes in front of the block and runs on into it",
          [lit(64), one(1, 40, 3)], [("seq", 0, 1, 0, {"pos": 1, "offset": 3, "ml": 40, "source": -2, "source_end": 38})])
    valid("history in a stored block", "the bytes a match copies were written by a stored block's copy",
          [("stored", 200), one(2, 16, 150)], [("block", 0, 0, {"stored": True, "size": 200}), ("seq", 0, 1, 0, {"source": -148, "source_end": -132})])
    valid("stored block between compressed ones", "a match over a stored block into the compressed block in front of it",
          [lit(90), ("stored", 33), one(4, 60, 100)], [("block", 0, 1, {"stored": True}), ("seq", 0, 2, 0, {"source": -96, "source_end": -36, "history": 123})])
    valid("four short blocks back", "a block of 100 bytes whose match begins in the first of four 20-byte blocks in front of it",
          [lit(20), lit(20), lit(20), lit(20), one(10, 60, 85, tail=30)],
          [("blocks", 0, 5, 65536)] + [("block", 0, k, {"size": 20}) for k in range(4)] + [("block", 0, 4, {"size": 100}), ("seq", 0, 4, 0, {"source": -75, "source_end": -15})])
    valid("source ends at the boundary", "a match whose source ends exactly at the block's first byte",
          [lit(100), one(3, 20, 23)], [("seq", 0, 1, 0, {"source": -20, "source_end": 0})])

    # ---- the output ring: OUT_RING bytes, LDS_REACH of them served from LDS, empty at a block's start ----
    for d in (LDS_REACH - 1, LDS_REACH, LDS_REACH + 1, OUT_RING - 1, OUT_RING, OUT_RING + 1):
        valid("source %d in front of the boundary" % d, "a block's first match begins %d bytes in front of the block (LDS_REACH %d, OUT_RING %d)" % (d, LDS_REACH, OUT_RING),
              [lit(5000), one(1, 24, d + 1)], [("seq", 0, 1, 0, {"pos": 1, "source": -d})])
        valid("match %d behind the boundary" % d, "a match written %d bytes behind the boundary whose source straddles it" % d,
              [lit(5000), one(d, 24, d + 7)], [("seq", 0, 1, 0, {"pos": d, "source": -7, "source_end": 17})])
    valid("far match from history into the block", "a match longer than its distance beyond LDS_REACH: the source begins in the block in front and runs on into this one",
          [lit(5000), one(10, 4100, 4000)], [("seq", 0, 1, 0, {"source": -3990, "source_end": 110})])
    valid("near periodic match across the boundary", "3 000 bytes at distance 100 from position 10",
          [lit(5000), one(10, 3000, 100)], [("seq", 0, 1, 0, {"source": -90, "source_end": 2910})])
    valid("history shorter than a granule", "three bytes of history, all of them matched",
          [lit(3), one(0, 19, 3)], [("seq", 0, 1, 0, {"history": 3, "source": -3})])

    # ---- the frame around linked blocks ----
    a, b = fr([lit(100), one(0, 8, 50)]), fr([one(4, 8, 10)])
    assert a.plain is not None and b.plain is None
    add("second frame reaches in front of itself", "two linked frames: the second frame's first block asks for bytes of the first frame's content -- which the "
        "destination holds -- and must fail", a.data + b.data, None, [("frames", [True, True]), ("seq", 1, 0, 0, {"pos": 4, "history": 0, "offset": 10, "ip": 7})], OFFSET_OUTSIDE, 7)
    b = fr([lit(60), one(2, 12, 40)])
    add("two linked frames and a skippable one", "concatenated linked frames with a skippable frame between them, each with a history of its own",
        a.data + ref.skippable(b"metadata") + b.data, a.plain + b.plain,
        [("frames", [True, True]), ("skippable", len(a.data)), ("seq", 0, 1, 0, {"source": -50}), ("seq", 1, 1, 0, {"source": -38})])
    c = fr([lit(70), one(10, 9, 5)], linked=False)
    add("independent frame, then a linked one", "the setting leaves the frames of independent blocks beside a linked one alone", c.data + a.data, c.plain + a.plain,
        [("frames", [False, True])])
    blocks = [lit(200), one(3, 30, 100, tail=20)]
    f = fr(blocks, block_checksum=True)
    add("block checksums", "block checksums over the stored bytes of linked blocks", f.data, f.plain, [("flag", 0, ref.FLG_BLOCK_CHECKSUM, True), ("frames", [True])])
    f = fr(blocks, block_checksum=True, bad_block_checksum=1)
    w = ref.walk(f.data)[0].blocks[1]
    add("damaged block checksum", "the second block's checksum is wrong", f.data, None, [("flag", 0, ref.FLG_BLOCK_CHECKSUM, True), ("frames", [True])],
        ref.malformed(ref.D_BLOCK_CHECKSUM), w.at + w.length)
    f = fr(blocks, content_checksum=True)
    add("content checksum", "a content checksum over a linked frame's content", f.data, f.plain, [("flag", 0, ref.FLG_CONTENT_CHECKSUM, True), ("frames", [True])])
    f = fr(blocks, content_checksum=True, bad_content_checksum=True)
    add("damaged content checksum", "the content checksum is wrong", f.data, None, [("flag", 0, ref.FLG_CONTENT_CHECKSUM, True), ("frames", [True])],
        ref.malformed(ref.D_CONTENT_CHECKSUM), len(f.data) - 4)
    f = fr(blocks, content_size=True)
    add("content size", "the content size of a linked frame, as announced", f.data, f.plain, [("flag", 0, ref.FLG_CONTENT_SIZE, True), ("frames", [True])])
    f = fr(blocks, content_size=252)
    add("wrong content size", "a linked frame announces one byte less than it holds", f.data, None, [("flag", 0, ref.FLG_CONTENT_SIZE, True), ("frames", [True])],
        ref.malformed(ref.D_CONTENT_SIZE), len(f.data))
    f = fr(blocks, dictionary=True)
    add("dictionary", "a linked frame with a dictionary ID is refused as one of independent blocks is", f.data, None, [("flag", 0, ref.FLG_DICTIONARY, True), ("frames", [True])],
        ref.malformed(ref.D_DICTIONARY), 4)
    f = fr(blocks)
    w = ref.walk(f.data)[0].blocks[1]
    add("capacity exact", "the output has exactly the content's room", f.data, f.plain, [("cap", 0), ("frames", [True])])
    add("capacity one short", "one byte less: the second block's last literals do not fit", f.data, None, [("cap", 1), ("frames", [True])],
        ref.malformed(ref.D_LZ4_LAST_LITERAL_OUTSIDE), w.tail_ip, cap=len(f.plain) - 1)
    add("capacity short by a block", "no room at all for the second block", f.data, None, [("cap", w.size), ("frames", [True])],
        ref.malformed(ref.D_OUTPUT_TOO_SMALL), 200, cap=len(f.plain) - w.size)
    f = fr([lit(200), ("stored", 53)])
    add("capacity short inside a stored block", "a stored block of a linked frame that does not fit", f.data, None, [("cap", 1), ("block", 0, 1, {"stored": True}), ("frames", [True])],
        ref.malformed(ref.D_OUTPUT_TOO_SMALL), 200, cap=len(f.plain) - 1)

    # ---- an encoder's frames ----
    plain = text(262144)
    f = fr(ref.greedy_blocks(plain, 65536, linked=True), content_checksum=True)
    assert f.plain == plain
    add("256 KiB of text, linked", "four 64 KiB blocks of a greedy encoder with one table over the whole content: matches across every boundary", f.data, plain,
        [("frames", [True]), ("blocks", 0, 4, 65536), ("cross", 0, 100)])
    f = fr(ref.greedy_blocks(plain, 65536, linked=False), linked=False, content_checksum=True)
    assert f.plain == plain
    add("256 KiB of text, independent", "the same content as a frame of independent blocks", f.data, plain, [("frames", [False]), ("blocks", 0, 4, 65536), ("contained", 0)],
        linked=False)
    f = fr([lit(50), one(0, 20, 1)], linked=False)
    assert f.plain is None
    add("independent frame with a reaching offset", "the first case's blocks under a set independence bit: the offset is outside, with the setting or without",
        f.data, None, [("frames", [False]), ("seq", 0, 1, 0, {"pos": 0, "offset": 1})], OFFSET_OUTSIDE, 3, linked=False)
    return out
