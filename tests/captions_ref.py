"""The caption rule of vlog_amd/captions.py restated in a straight line, for tests/test_captions_host.py.

The generator there makes one pass and decides line and cue at every word.  Here a cue is found in two steps from
the word it starts at: first ALL its candidate lines are laid out by width alone (at most max_line_count of them),
then the laid-out words are cut at the first one before which a pause, the duration limit or a sentence end asks
for a new cue.  Plain tuples in, plain dicts out; nothing is shared with the module under test but the two constants
that the rule names (the 3.0 s pause is written out)."""
from typing import List, Optional, Sequence, Tuple

SENTENCE_END = ".?!。？！"
PAUSE_S = 3.0


def ref_cues(words: Sequence[Tuple[str, float, float, Sequence[int]]], width: int, count: int,
             seconds: Optional[float]) -> List[dict]:
    """words: one parent's (text, start, end, tokens) -> [dict(lines, words=[indices into words], start, end, tokens)]"""
    idx = [k for k, w in enumerate(words) if w[0]]
    text = lambda ks: "".join(words[k][0] for k in ks)
    out = []
    p = 0
    while p < len(idx):
        # step 1: every line this cue could hold, by width alone
        lines = [[idx[p]]]
        for k in idx[p + 1:]:
            if len((text(lines[-1]) + words[k][0]).strip()) <= width:
                lines[-1].append(k)
            elif len(lines) < count:
                lines.append([k])
            else:
                break
        laid = [k for line in lines for k in line]
        # step 2: the first laid-out word that has to start a cue of its own cuts the layout
        keep = len(laid)
        for j in range(1, len(laid)):
            k, prev = laid[j], laid[j - 1]
            before = "\n".join(text([q for q in line if q < k]).strip() for line in lines if line[0] < k)
            last = words[prev][0].strip()
            if words[k][1] - words[prev][2] > PAUSE_S \
                    or (seconds is not None and words[k][2] - words[laid[0]][1] > seconds) \
                    or (last and last[-1] in SENTENCE_END and 2 * len(before) >= width * count):
                keep = j
                break
        mine = laid[:keep]
        out.append(dict(lines=[text([q for q in line if q in mine]).strip() for line in lines if line[0] in mine],
                        words=mine, start=words[mine[0]][1], end=words[mine[-1]][2],
                        tokens=[t for k in mine for t in words[k][3]]))
        p += keep
    return out
