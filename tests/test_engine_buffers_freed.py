"""Every device buffer the engine owns is released by wm_destroy: DevBuf has no destructor, so a member that is missing
from wm_destroy's release list leaks for the life of the process (the fp8 K/V panels' exponent bytes and staging
buffer are several hundred MB at large-v3).  csrc/engine.cpp is read as text; no GPU and no library."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def engine_text():
    return (ROOT / "vlog_amd" / "csrc" / "engine.cpp").read_text()


def declared_buffers(text):
    """Names of the DevBuf members of struct wm_engine (nested structs' members are released where they live)."""
    start = text.index("struct wm_engine {")
    end = text.index("\n};", start)
    body, depth, names = text[start:end], 0, []
    for line in body.splitlines()[1:]:
        code = line.split("//")[0]
        if depth == 0:
            m = re.match(r"\s*DevBuf\s+([^;*&()]+);", code)
            if m:
                names += [n.strip() for n in m.group(1).split(",")]
        depth += code.count("{") - code.count("}")
    return names


def released_buffers(text):
    start = text.index("void wm_destroy(wm_engine* e) {")
    end = text.index("\n}\n", start)
    return set(re.findall(r"&e->(\w+)", text[start:end]))


def test_wm_destroy_releases_every_device_buffer():
    text = engine_text()
    declared = declared_buffers(text)
    assert len(declared) >= 60 and "ckv" in declared and "arena" in declared      # the parse found the struct
    assert {"ckv_exp", "kv8_stage"} <= set(declared)
    missing = sorted(set(declared) - released_buffers(text))
    assert not missing, f"wm_destroy does not release: {missing}"
