"""CPU tests (-m "not gpu") of the development switches' one list: enum sz3hip_dbg (include/sz3hip_debug.h) and sz3_amd.Dbg name the
same switches with the same values, the bits that carry several meanings are exactly the known ones, the library's sources test the
switches by name only, and sz3_amd.debug_flags sets the word for its body alone; the block decoder's read-out (enum sz3hip_blkdec_form /
sz3hip_blkdec_word, sz3hip_debug_blkdec_last) is listed the same way in the header, in Python and in the library. No device needed."""
import os
import re

import pytest

import sz3_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sz3_amd", "csrc")

# the bits with several meanings (names without the prefix); everything else has its bit to itself
SHARED = {
    1: {"CB_COMPACT_IN_WG", "K1_LAB_NO_HIST"},
    2: {"DEC_MULTI_SYM", "K1_NO_CODE_STORES"},
    4: {"BLKDEC_FORCE_RETRY", "K1_V4_NO_STENCIL"},
    16: {"BLKDEC_LOCAL_EXPANDED", "K1_V4_NO_PREFETCH", "PACK_LAB_NO_STORES"},
    512: {"DEC_NO_FUSED_X", "PACK_LAB_ONE_UNIT"},
    2048: {"K1_NO_FUSED", "BLK_RANK_3_LAUNCHES", "BLK_SIDE_8_LAUNCHES"},
    4096: {"K1_NO_XCD_ORDER", "CB_NO_SPEC_WIDE"},
    32768: {"PACK_OLD", "BLKDEC_GROUPS_3"},
    65536: {"CB_NO_SAMPLED", "BLKDEC_PER_FRONT"},
    4194304: {"INTERP_LEVELS_ANY_SIZE", "K1_NO_SAMP_IN_LAUNCH"},
    8388608: {"BLKDEC_BLOCK_PER_WAVE", "K1_Q16_PLAIN_STORES"},
    536870912: {"INTERP_HANDOVER_IN_PLACE", "DEC_CARRY_PASS"},
}
AREAS = ("K1", "PACK", "CB", "DEC", "INTERP", "BLK", "BLKDEC", "CTX")


def _header_enumerators():
    """{name without SZ3HIP_DBG_: value as an unsigned 32-bit word} from the header's text. The initialisers are decimal literals but
    for bit 31, which a C enumerator (an int) can only spell as INT_MIN: `-2147483647 - 1`."""
    txt = open(os.path.join(ROOT, "include", "sz3hip_debug.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    body = re.search(r"enum\s+sz3hip_dbg\s*\{(.*?)\}", txt, flags=re.S).group(1)
    out = {}
    for item in body.split(","):
        item = item.strip()
        if not item:
            continue
        m = re.fullmatch(r"SZ3HIP_DBG_([A-Z0-9_]+)\s*=\s*([-0-9 ]+)", item)
        assert m, "not `SZ3HIP_DBG_<NAME> = <decimal>`: %r" % item
        assert m.group(1) not in out, "listed twice: " + m.group(1)
        terms = m.group(2).replace(" ", "").replace("-", " -").split()
        out[m.group(1)] = sum(int(t) for t in terms) & 0xFFFFFFFF
    return out


def test_header_and_python_enum_agree():
    hdr = _header_enumerators()
    py = {name: int(member) for name, member in sz3_amd.Dbg.__members__.items()}  # (__members__: the aliases of shared bits too)
    assert hdr == py, {"header only": sorted(set(hdr) - set(py)), "python only": sorted(set(py) - set(hdr)),
                       "values differ": sorted(k for k in set(hdr) & set(py) if hdr[k] != py[k])}
    for name, v in hdr.items():
        assert v != 0 and v & (v - 1) == 0, "%s = %d is not exactly one bit" % (name, v)
        assert name.split("_")[0] in AREAS, name


def test_shared_bits_are_the_known_ones():
    groups = {}
    for name, v in _header_enumerators().items():
        groups.setdefault(v, set()).add(name)
    assert {v: g for v, g in groups.items() if len(g) > 1} == SHARED


def test_all_32_bits_are_in_use():
    union = 0
    for v in _header_enumerators().values():
        union |= v
    assert union == 0xFFFFFFFF


def test_sources_test_the_switches_by_name():
    """no numeric test of the flag word (szk_dbg_flags, a local dbg copy, p.dbg / c.p->dbg) and no decimal literal ORed into it"""
    numeric = re.compile(r"dbg(_flags)?\s*[&|]\s*\(?\s*[0-9]"        # dbg_flags & 256, p.dbg & 4u, ->dbg & 1u, dbg & (32768 ...
                         r"|dbg(_flags)?\b[^;\n]*?[|&]\s*[0-9]+u?\s*[|&,)]")  # ... | 65536) inside a mask, szk_dbg_flags | 32768 | 65536, as an argument
    hits = []
    for fn in sorted(os.listdir(CSRC)):
        for no, line in enumerate(open(os.path.join(CSRC, fn), errors="replace"), 1):
            if numeric.search(line):
                hits.append("%s:%d: %s" % (fn, no, line.strip()[:160]))
    assert not hits, "\n".join(hits)


class _StubLib:
    def __init__(self):
        self.word = None
        self.calls = []

    def sz3hip_debug_flags(self, flags):
        assert type(flags) is int  # (what crosses into ctypes is a plain int)
        self.word = flags
        self.calls.append(flags)


def test_debug_flags_context_manager(monkeypatch):
    stub = _StubLib()
    monkeypatch.setattr(sz3_amd, "lib", lambda: stub)
    D = sz3_amd.Dbg
    with sz3_amd.debug_flags(D.BLK_NO_EXIT | D.BLK_NO_SELECT):
        assert stub.word == 1073741824 + 2147483648
    assert stub.word == 0 and stub.calls == [3221225472, 0]
    with pytest.raises(KeyError):
        with sz3_amd.debug_flags(D.K1_NO_Q16):
            assert stub.word == 8
            raise KeyError("body")
    assert stub.word == 0 and stub.calls == [3221225472, 0, 8, 0]
    with sz3_amd.debug_flags(0):
        assert stub.word == 0
    assert stub.word == 0


def _header_enum(name, prefix):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sz3hip_debug.h")).read(), flags=re.S)
    body = re.search(r"enum\s+%s\s*\{(.*?)\}" % name, txt, flags=re.S).group(1)
    return {m.group(1): int(m.group(2)) for m in re.finditer(prefix + r"([A-Z0-9_]+)\s*=\s*(\d+)", body)}


def test_block_decoder_read_out_is_listed():
    """the forms: header and sz3_amd.BlkDecForm agree, values 0 .. 11 once each; the words: the accessor's keys in the header's order;
    the library exports the call, and before any block stream was decoded it reports nothing"""
    forms = _header_enum("sz3hip_blkdec_form", "SZ3HIP_BLKDEC_FORM_")
    assert forms == {name: int(v) for name, v in sz3_amd.BlkDecForm.__members__.items()}
    assert sorted(forms.values()) == list(range(12)) and forms["NONE"] == 0
    words = _header_enum("sz3hip_blkdec_word", "SZ3HIP_BLKDEC_WORD_")
    assert sorted(words.values()) == list(range(7))
    L = sz3_amd.lib()
    assert hasattr(L, "sz3hip_debug_blkdec_last")
    info = sz3_amd.debug_blkdec_last()
    assert [k.upper() for k in info] == sorted(words, key=words.get)
    assert info["form"] == sz3_amd.BlkDecForm.NONE and not any(info.values())
