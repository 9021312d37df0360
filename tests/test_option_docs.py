"""The engine options documented in include/whisper_mi355.h are the ones the engine has: the quoted keys of the
header's option comment and the keys of the option table in csrc/engine.cpp (kOptions) are the same set.  Both
files are read as text; no GPU and no library."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PER_PROJECTION = {"decode_gemm.<proj>", "decode_gemm_cols.<proj>"}     # explicit code beside the table
PROJECTIONS = ("qkv", "out", "cq", "cout", "fc1", "fc2")


def header_option_keys():
    """Every quoted key of the option comment (the comment that ends at wm_set_option's declaration)."""
    text = (ROOT / "include" / "whisper_mi355.h").read_text()
    start = text.index("/* Engine options")
    end = text.index("int wm_set_option(", start)
    return set(re.findall(r'"([a-z0-9_]+(?:\.<proj>)?)"', text[start:end]))


def table_option_keys():
    text = (ROOT / "vlog_amd" / "csrc" / "engine.cpp").read_text()
    start = text.index("const OptRow kOptions[] = {")
    end = text.index("\n};", start)
    keys = re.findall(r'^\s*\{"([a-z0-9_]+)",', text[start:end], flags=re.M)
    assert len(keys) == len(set(keys)), "a key appears twice in kOptions"
    return set(keys)


def test_header_documents_exactly_the_table():
    header, table = header_option_keys(), table_option_keys()
    assert len(table) >= 20                       # the parse found the table, not a fragment of it
    assert PER_PROJECTION <= header
    assert header - PER_PROJECTION == table, (sorted(header - PER_PROJECTION - table), sorted(table - header))
