"""Text normalisation used before WER/CER (same `VOCAB_SPECS` / `normalize_text` interface as the reference's
eval/utils.py:7-111).  The character classes are data: v0 = lower-case a-z, digits, umlauts, space (Swiss-German
ASR convention); v1-v3 keep case and add punctuation."""
from __future__ import annotations

import re
import string
from typing import Dict, Sequence, Set

_SPACES = re.compile(r"[ \t]+")

_FOLD_BASE = dict(zip("áàâçéèêíìîñóòôúùûșş", "aaaceeeiiinooouuuss"))
_LOOKUP_V0 = {**_FOLD_BASE, "ß": "ss", "-": " ", "–": " ", "/": " "}
_LOOKUP_V1 = {**_LOOKUP_V0, **{k.upper(): v.upper() for k, v in _LOOKUP_V0.items()}}
_LOOKUP_V3 = {**{k: v for k, v in _FOLD_BASE.items() if k != "ş"}, "ß": "ss", "–": "-", "\xad": "-"}

_LOWER = string.ascii_lowercase + string.digits
_BOTH = string.ascii_lowercase + string.ascii_uppercase + string.digits

VOCAB_SPECS = {
    "v0": {"char_vocab": set(_LOWER + "äöü "), "char_lookup": _LOOKUP_V0, "transform_lowercase": True},
    "v1": {"char_vocab": set(_BOTH + "äöüÄÖÜ" + " .,:"), "char_lookup": _LOOKUP_V1, "transform_lowercase": False},
    "v2": {"char_vocab": set(_LOWER + "äöü" + " .,:"), "char_lookup": _LOOKUP_V1, "transform_lowercase": False},
    "v3": {"char_vocab": set(_BOTH + "äöüÄÖÜ" + " .,:-?!;"), "char_lookup": _LOOKUP_V3, "transform_lowercase": False},
}


def normalize_text(text: str, char_vocab: Set[str], char_lookup: Dict[str, str], transform_lowercase: bool = True) -> str:
    """lower-case (optional) -> fold characters via the lookup -> collapse blanks -> drop out-of-vocabulary
    characters -> collapse blanks again -> strip."""
    if transform_lowercase:
        text = text.lower()
    for src, dst in char_lookup.items():
        text = text.replace(src, dst)
    text = _SPACES.sub(" ", text)
    text = "".join(ch for ch in text if ch in char_vocab)
    return _SPACES.sub(" ", text).strip()


def decode_prefix_len(y_in: Sequence[int], sot: int, no_timestamps: int, with_timestamps: bool = False) -> int:
    """Length of the decoding prefix of one teacher-forcing input row: everything up to and including its start-of-transcript
    sequence — an optional prompt, then `sot`, language, task, and `no_timestamps` when it follows (a `no_speech` marker is not
    part of it).  The writer it agrees with: data/data_loader.py AudioDataset._get_special_tokens (prompt + specials + text).
    with_timestamps (decoding under the timestamp rules): the prefix stops behind the task token, a `no_timestamps` that follows
    is not part of it."""
    y = [int(t) for t in y_in]
    if sot not in y:
        raise ValueError("no start-of-transcript token in the decoder input")
    n = y.index(sot) + 3  # sot, <|language|>, <|task|>: a prompt holds text and sot_prev only, so the first sot is THE sot
    if n > len(y):
        raise ValueError("the decoder input ends inside its start-of-transcript sequence")
    if not with_timestamps and n < len(y) and y[n] == no_timestamps:
        n += 1
    return n
