"""MK_GUNZIP_REPAIR in plain Python, on top of gunzip_model's finder and piece decode: the rule by which the host
repairs false piece starts, and the streams with planted false starts that tests/test_gunzip_repair_model.py holds against zlib and
tests/test_gpu_gunzip_repair.py against the device.

The rule, for the pieces in stream order.  The stream's first piece is confirmed; piece k + 1 is confirmed when piece k is and
stopped at its start with OK.  For a confirmed piece with `end` (the next start) and `stop` (the bit its decode stopped at):
  OK         the next piece is confirmed
  MISSED     (in front of a block header, stop > end) every start s with end <= s < stop is dropped, stop becomes a start unless it
             is one, and the piece is OK with end = stop and the symbols it gave
  CAPACITY   not the stream's last piece: the next start is dropped and the piece decoded again from its start with
             ratio * (bytes of the merged range) symbols, MERGES times at the most; then CAPACITY stands
  any other  is the stream's status
`repairs` counts the starts dropped.  A piece's decode depends on its start, its end and its capacity alone, so the order in which
the device decodes pieces, its batches included, changes nothing: the model decodes one piece after the other."""
import random
import zlib

import bgzf_util as bu
import gunzip_model as gm
from gunzip_model import CAPACITY, MISSED, OK, WINDOW

MERGES = 8  # MK_GUNZIP_REPAIR_MERGES


def run(raw, span, ratio=1 << 20):
    """-> (status, text, pieces, repairs): gunzip_model.run with the repair; pieces = [(start bit, symbols)], the final ones, as far
    as they were decoded, the piece whose status stands included"""
    starts = [0] + gm.find_candidates(raw, span)
    window = bytearray(WINDOW)
    text, table, repairs, k = bytearray(), [], 0, 0
    while k < len(starts):
        start, merges = starts[k], 0
        while True:
            end = starts[k + 1] if k + 1 < len(starts) else None
            st, syms, stop = gm.decode_piece(raw, start, end, gm.piece_cap(raw, start, end, ratio), k == 0, end is None)
            if st == MISSED and stop > end:
                j = k + 1
                while j < len(starts) and starts[j] < stop:
                    j += 1
                repairs += j - (k + 1)
                del starts[k + 1:j]
                if not (k + 1 < len(starts) and starts[k + 1] == stop):
                    starts.insert(k + 1, stop)
                st = OK
            elif st == CAPACITY and end is not None and merges < MERGES:
                del starts[k + 1]
                repairs += 1
                merges += 1
                continue
            break
        table.append((start, len(syms)))
        if st:
            return st, None, table, repairs
        piece = bytes(s if s < 0x8000 else window[s & 0x7fff] for s in syms)
        text += piece
        window = (window + piece)[-WINDOW:]
        k += 1
    return OK, bytes(text), table, repairs


# ---- streams with planted false starts ------------------------------------------------------------------------------------------------

SPAN = 1024


def header_image():
    """the bytes of a valid non-final dynamic block header (tests/test_gpu_gunzip.py's missed_stream plants the same)"""
    w = bu.BitWriter()
    bu.dynamic_block(w, bu.spread(257, {65: 2, 66: 2, 67: 2, 256: 2}), [1, 1], [], 0, stop="ops")
    image = w.done()
    assert b"\n" not in image and b"\r" not in image and b"\0" in image and len(image) == 42
    return image


def missed_stream():
    """tests/test_gpu_gunzip.py's missed_stream(): the image in a stored block at payload byte 1030, then a final fixed block"""
    image = header_image()
    data = bytearray(b"\xff" * 3000)
    data[1025:1025 + len(image)] = image
    w = bu.BitWriter()
    bu.stored_block(w, bytes(data), 0)
    bu.fixed_block(w, list(b"@r\nACGT\n+\nIIII\n"), 1)
    raw = w.done()
    return raw, zlib.decompress(raw, -15), [8 * 1030]


def record(rng, name, n, seq=None):
    """a FASTQ record with n bases; 16 quality values around 53, so that deflate gives less than 4 bytes of text a compressed byte
    and a -Q 53 masks one base in sixteen"""
    seq = seq or bytes(rng.choice(b"ACGT") for _ in range(n))
    qual = bytes(rng.choice(b"3579;=?ACEGIKMOQ") for _ in range(len(seq)))
    return b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def records(rng, tag, nbytes):
    """every third read is the one in front of it once more, with qualities of its own: k-mers that occur twice"""
    out, i, seq = b"", 0, None
    while len(out) < nbytes:
        seq = seq if i % 3 == 2 else bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(60, 260)))
        out += record(rng, b"%s.%d" % (tag, i), 0, seq)
        i += 1
    return out


def stored_part(rng, at, nimages, nfill, short=False):
    """FASTQ records for ONE stored block whose bytes start at payload byte `at`: a record in front, `nimages` records whose `@`
    line ends in the header image, each image at the first byte of a span of its own (consecutive spans), `nfill` bytes of records
    behind.  short: the image record ends inside the image's span -> (text, [the images' payload bits])"""
    image = header_image()
    out = record(rng, b"stored.0", 80)
    bits = []
    for i in range(nimages):
        pad = -(at + len(out) + 1) % SPAN if i == 0 else SPAN - (1 + len(image) + 1 + 2 * 400 + 4)
        bits.append(8 * (at + len(out) + 1 + pad))
        out += record(rng, b"r" * pad + image, 100 if short else 400)
    out += records(rng, b"fill", nfill) if nfill else b""
    assert len(out) <= 40000 and all(b % (8 * SPAN) == 0 for b in bits) and bits == list(range(bits[0], bits[0] + 8 * SPAN * nimages, 8 * SPAN))
    return out, bits


def planted(seed, parts):
    """parts: ("deflate", text bytes) and ("stored", nimages, nfill, short) in turn, the last one a deflate part
    -> (raw, text, [planted bits])"""
    rng = random.Random(seed)
    raw, text, bits = b"", b"", []
    for i, part in enumerate(parts):
        if part[0] == "deflate":
            t = records(rng, b"p%d" % i, part[1])
            raw += gm.deflate(t, 6, 1, finish=i == len(parts) - 1)
        else:
            t, b = stored_part(rng, len(raw) + 5, *part[1:])
            raw += gm.stored_stretch(t, 40000)
            bits += b
        text += t
    assert parts[-1][0] == "deflate" and zlib.decompress(raw, -15) == text and len(raw) <= 65536
    return raw, text, bits


def four_images():
    """dynamic blocks, ONE stored block with the image in four consecutive spans and 24 KB of records behind them, dynamic blocks"""
    return planted(1, [("deflate", 16000), ("stored", 4, 24000, False), ("deflate", 24000)])


def two_rounds():
    """two stored blocks with one image each and dynamic blocks between them; each stored block ends inside its image's span, so
    the block start behind it is no candidate of the finder's: the repair has to start a piece there, twice"""
    return planted(2, [("deflate", 9000), ("stored", 1, 0, True), ("deflate", 14000), ("stored", 1, 0, True), ("deflate", 9000)])


def plain(text):
    """the same text without images: what a repaired stream must equal"""
    return gm.deflate(text, 6, 1)
