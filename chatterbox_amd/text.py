"""Host-side text front-end (CPU string work, microseconds; out of the kernel scope -- SURVEY.md section 2).

`punc_norm` follows the behaviour of the reference helper (mtl_tts.py:71-110); `MTLTokenizer` is the generic path
of the reference tokenizer wrapper (models/tokenizers/tokenizer.py:255-305: lowercase + NFKD + `[lang]` tag +
`[SPACE]` substitution + a `tokenizers` BPE).  The optional language-specific normalisers (Cangjie, kakasi, Hangul
decomposition, Hebrew diacritics, Russian stress) depend on third-party packages and data files that are not part
of the hot path; they are not re-implemented here and a warning is emitted when such a language is requested.
"""
import logging
import re
import unicodedata

import torch

log = logging.getLogger(__name__)

_PUNC_MAP = {"...": ", ", "…": ", ", ":": ",", " - ": ", ", ";": ", ", "—": "-", "–": "-", " ,": ",",
             "“": '"', "”": '"', "‘": "'", "’": "'"}
_ENDERS = (".", "!", "?", "-", ",", "、", "，", "。", "？", "！")
_NEEDS_EXTRA = {"zh", "ja", "he", "ko", "ru"}


def punc_norm(text: str, enders=_ENDERS) -> str:
    """Multilingual variant (mtl_tts.py:71-110): sentence enders include the CJK marks."""
    if not text:
        return "You need to add some text for me to talk."
    if text[0].islower():
        text = text[0].upper() + text[1:]
    text = " ".join(text.split())
    for old, new in _PUNC_MAP.items():
        text = text.replace(old, new)
    text = text.rstrip(" ")
    if not text.endswith(enders):
        text += "."
    return text


def punc_norm_en(text: str) -> str:
    """English ChatterboxTTS variant (tts.py:26-61): same replacement table, ASCII-only sentence enders."""
    return punc_norm(text, enders=(".", "!", "?", "-", ","))


_TURBO_PUNC_MAP = {"…": ", ", ":": ",", "—": "-", "–": "-", " ,": ",", "“": '"', "”": '"', "‘": "'", "’": "'"}


def punc_norm_turbo(text: str) -> str:
    """The Turbo/Nano variant of the helper (reference tts_turbo.py:30-66): a shorter replacement table, ASCII enders."""
    if not text:
        return "You need to add some text for me to talk."
    if text[0].islower():
        text = text[0].upper() + text[1:]
    text = " ".join(text.split())
    for old, new in _TURBO_PUNC_MAP.items():
        text = text.replace(old, new)
    text = text.rstrip(" ")
    if not text.endswith((".", "!", "?", "-", ",")):
        text += "."
    return text


class MTLTokenizer:
    SOT, EOT, SPACE = "[START]", "[STOP]", "[SPACE]"

    def __init__(self, vocab_file_path):
        from tokenizers import Tokenizer
        self.tokenizer = Tokenizer.from_file(str(vocab_file_path))
        voc = self.tokenizer.get_vocab()
        assert self.SOT in voc and self.EOT in voc, "tokenizer vocabulary lacks [START]/[STOP]"

    def encode(self, txt, language_id=None, lowercase=True, nfkd_normalize=True):
        if lowercase:
            txt = txt.lower()
        if nfkd_normalize:
            txt = unicodedata.normalize("NFKD", txt)
        if language_id in _NEEDS_EXTRA:
            log.warning("language '%s' uses an optional third-party normaliser in the reference that is not bundled; "
                        "falling back to the generic grapheme path", language_id)
        if language_id:
            txt = f"[{language_id.lower()}]{txt}"
        return self.tokenizer.encode(txt.replace(" ", self.SPACE)).ids

    def text_to_tokens(self, text, language_id=None, **kw):
        return torch.IntTensor(self.encode(text, language_id=language_id, **kw)).unsqueeze(0)

    def pieces(self, ids):
        """The vocabulary strings of token ids, one per id (word_groups' input); an id outside the vocabulary is the empty string"""
        return [self.tokenizer.id_to_token(int(i)) or "" for i in ids]


class EnTokenizer(MTLTokenizer):
    def encode(self, txt, language_id=None, **kw):
        return self.tokenizer.encode(txt.replace(" ", self.SPACE)).ids


# ---------------------------------------------------------------------------------------------------------------- word timestamps: text tokens -> words
def _is_special(piece):
    """[START], [STOP], a language tag: a bracketed name is a control token, not text"""
    return len(piece) > 2 and piece[0] == "[" and piece[-1] == "]"


def _is_punctuation(piece):
    return bool(piece) and all(unicodedata.category(c)[0] == "P" for c in piece)


def word_groups(pieces, space="[SPACE]"):
    """Group the text-token strings of one utterance into words: a list of (a, b), word k = pieces[a:b], in text order.  A `space` token ends a word and belongs
    to none; neither do control tokens (bracketed names: [START], [STOP], a language tag) or empty strings.  A piece that is only punctuation attaches to the
    word before it, also across a space ("hello , world": the comma joins "hello", whose range then spans the space); with no word before it, it starts one.
    A text without spaces is one word.  Pure host function: no tokenizer, no tensors."""
    groups, open_ = [], False
    for i, p in enumerate(pieces):
        if p == space or not p or _is_special(p):
            open_ = False
        elif open_ or (groups and _is_punctuation(p)):
            groups[-1] = (groups[-1][0], i + 1)
        else:
            groups.append((i, i + 1))
            open_ = True
    return groups


# ---------------------------------------------------------------------------------------------------------------- long-form synthesis: text -> chunks
# The reference synthesises at most 1000 speech tokens per call (tts.py:249, mtl_tts.py:328: 40 s at 25 tokens/s) and cuts a longer text off; generate_long
# (api.py) speaks a text of any length as consecutive chunks.  DEFAULT_MAX_CHARS: characters per chunk -- 300, and 100 for zh / ja / ko, from that rate and cap with
# a 2x margin.  UNMEASURED: nobody has checked these against trained weights; generate_long reports every chunk whose tokens ran into the cap.
DEFAULT_MAX_CHARS, DEFAULT_MAX_CHARS_CJK = 300, 100
CJK_LANGUAGES = ("zh", "ja", "ko")
_PARAGRAPH = re.compile(r"\n\s*\n")
# a run of . ! ? ... and closing quotes / brackets in front of whitespace or the end (so "3.14" and "e.g.x" do not split); a run of the CJK marks, whatever follows
_SENTENCE_END = re.compile(r"[.!?…]+[\"'”’»)\]}]*(?=\s|$)|[。！？]+[\"'”’»」』）)\]}]*")
_CLAUSE_MARKS = ",;:、，"


def default_max_chars(cjk=False):
    return DEFAULT_MAX_CHARS_CJK if cjk else DEFAULT_MAX_CHARS


def _cut_long(s, max_chars):
    """Where to cut a sentence s (no outer whitespace, len(s) > max_chars): behind the last clause mark (, ; : 、 ， or " - ") that leaves at most max_chars
    characters, else at the last whitespace, else at max_chars.  -> cut in [1, max_chars]; s[:cut] is not blank."""
    cut = max((i + 1 for i in range(max_chars) if s[i] in _CLAUSE_MARKS), default=0)
    dash = s.rfind(" - ", 0, max_chars)
    cut = max(cut, dash + 2 if dash > 0 else 0)
    if cut == 0:
        cut = max((i for i in range(1, max_chars + 1) if s[i].isspace()), default=0)
    return cut or max_chars


def split_text(text, max_chars=None, cjk=False):
    """text -> [(chunk, paragraph_end), ...] for generate_long: pure string work, deterministic.
      * paragraphs end at blank lines; a chunk never crosses one; paragraph_end marks the last chunk of every paragraph but the final one;
      * inside a paragraph a sentence ends behind a run of . ! ? ... (closing quotes / brackets may follow) in front of whitespace or the paragraph's end, and
        behind a run of the CJK marks whatever follows;
      * consecutive sentences are packed greedily into one chunk while it stays <= max_chars (which keeps "Dr. Smith" together in practice);
      * a sentence longer than max_chars is cut behind its last clause mark inside the limit, else at the last whitespace, else at max_chars.
    No chunk is blank or longer than max_chars, every chunk is stripped, and the chunks hold the text's non-whitespace characters in order.  A blank text gives
    one empty chunk (the normalisers then speak their fallback sentence, as generate("") does).  max_chars=None: default_max_chars(cjk) -- an unmeasured choice."""
    if not isinstance(text, str):
        raise TypeError(f"text: expected a str, got {type(text).__name__}")
    if max_chars is None:
        max_chars = default_max_chars(cjk)
    if isinstance(max_chars, bool) or not isinstance(max_chars, int):
        raise TypeError(f"max_chars: expected an int, got {type(max_chars).__name__}")
    if max_chars < 1:
        raise ValueError(f"max_chars = {max_chars}: expected an int >= 1")
    out = []
    for para in _PARAGRAPH.split(text):
        units, lo = [], 0  # [start, end) of sentences and of the pieces of over-long ones, without outer whitespace
        for hi in [m.end() for m in _SENTENCE_END.finditer(para)] + [len(para)]:
            a, b = lo, hi
            lo = hi
            while a < b and para[a].isspace():
                a += 1
            while b > a and para[b - 1].isspace():
                b -= 1
            while b - a > max_chars:
                c = a + _cut_long(para[a:b], max_chars)
                e = c
                while para[e - 1].isspace():
                    e -= 1
                units.append((a, e))
                a = c
                while a < b and para[a].isspace():
                    a += 1
            if b > a:
                units.append((a, b))
        chunks, cur = [], None
        for a, b in units:
            if cur is not None and b - cur[0] <= max_chars:
                cur = (cur[0], b)
            else:
                if cur is not None:
                    chunks.append(cur)
                cur = (a, b)
        if cur is not None:
            chunks.append(cur)
        if chunks and out:
            out[-1] = (out[-1][0], True)
        out += [(para[a:b], False) for a, b in chunks]
    return out or [("", False)]
