"""The groups-file parser of `lash merge` (csrc/host/merge.cpp: parse_groups) through its hook in liblash_host.so.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import host_lib as H

_fn = H.lib.lash_host_parse_groups
_fn.restype = C.c_void_p
_fn.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p),
                C.POINTER(C.c_void_p)]

NAMES = ["a.fa", "b.fa", "c.fa", "rec1", "d e.fa", "rec1", "f.fa", "rec1"]


def parse(text, names=NAMES):
    """-> [(group name, [member indices])]; raises ValueError with the parser's message"""
    raw = text if isinstance(text, bytes) else text.encode()
    gn, off, mem, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    err = _fn(raw, len(raw), "\n".join(names).encode(), len(names), C.byref(gn), C.byref(n), C.byref(off), C.byref(mem))
    if err:
        raise ValueError(H._take_str(err))
    groups = H._take_str(gn).split("\n")[:n.value]
    o = np.frombuffer(C.string_at(off, 8 * (n.value + 1)), dtype=np.uint64).astype(np.int64)
    m = np.frombuffer(C.string_at(mem, 4 * int(o[-1])), dtype=np.uint32)
    H.lib.lash_host_free(off)
    H.lib.lash_host_free(mem)
    assert o[0] == 0 and len(groups) == n.value
    return [(g, m[o[i]:o[i + 1]].tolist()) for i, g in enumerate(groups)]


def test_cluster_output_is_read_as_it_is():
    text = "Representative\tMember\na.fa\ta.fa\na.fa\tb.fa\nc.fa\tc.fa\na.fa\tf.fa\n"
    assert parse(text) == [("a.fa", [0, 1, 6]), ("c.fa", [2])]
    assert parse(text[len("Representative\tMember\n"):]) == parse(text)                   # the heading is optional ...
    with pytest.raises(ValueError, match=r"line 3: 'Member' is not a name"):                # ... and a heading only on the first line
        parse("a.fa\ta.fa\nc.fa\tc.fa\nRepresentative\tMember\n")


def test_cr_blank_lines_and_a_missing_last_newline():
    assert parse("g1\ta.fa\r\n\r\n\ng2\td e.fa\r\ng1\tc.fa") == [("g1", [0, 2]), ("g2", [4])]
    with pytest.raises(ValueError, match=r"line 3: 'Member' is not a name"):                # blank lines count; a heading on line 3 is a member line
        parse("\n\nRepresentative\tMember\n")


def test_a_name_several_sketches_carry_selects_all_of_them():
    assert parse("bin\trec1\nbin\ta.fa\n") == [("bin", [3, 5, 7, 0])]


def test_first_appearance_order_overlaps_and_repeats():
    got = parse("z\tc.fa\ny\ta.fa\nz\ta.fa\nx\tf.fa\ny\ta.fa\ny\tb.fa\n")
    assert got == [("z", [2, 0]), ("y", [0, 0, 1]), ("x", [6])]


def test_names_are_whole_strings():
    assert parse("g\td e.fa\n") == [("g", [4])]
    with pytest.raises(ValueError, match=r"line 1: 'd' is not a name"):
        parse("g\td\n")
    with pytest.raises(ValueError, match=r"line 1: ' a.fa' is not a name"):
        parse("g\t a.fa\n")


@pytest.mark.parametrize("text,msg", [
    ("g\ta.fa\nno tab here\n", r"line 2: no tab"),
    ("g\ta.fa\n\ng\ta.fa\tb.fa\n", r"line 3: more than one tab"),
    ("Representative\tMember\n\ta.fa\n", r"line 2: empty group name"),
    ("g\ta.fa\r\ng\t\r\n", r"line 2: empty member name"),
    ("g\ta.fa\ng\tb.fa\ng\tnope.fa\n", r"line 3: 'nope.fa' is not a name of the collection"),
    ("", r"no group"),
    ("Representative\tMember\n\n\r\n", r"no group"),
])
def test_refusals_name_the_line(text, msg):
    with pytest.raises(ValueError, match=msg):
        parse(text)
