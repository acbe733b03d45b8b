"""Byte-level BPE tokenizer of CLIP's text tower for ASCII class names (what `tokenize` of the reference's core/model/backbone/clip.py:639-665 produces
for them): html-unescape, whitespace cleaning, lower-casing, the split into words / digits / punctuation runs, the merges in rank order, the start
and end tokens, zero padding to the context length, and truncation that cuts the end token off (clip.py:661-662 does).

The merges file (`bpe_simple_vocab_16e6.txt.gz`, 1.3 MB, OpenAI's) is NOT part of this repository: its path comes from the `bpe_path` argument or
$CLHIP_CLIP_BPE, and a missing file is an error that says so.  `ftfy` is not required: text that is not ASCII after unescaping is refused instead of
being repaired.  Callers without the file pass pre-tokenized `class_tokens` to the classifier.

Token ids: the 256 byte symbols in the order printable ASCII, the Latin-1 printable ranges, then the rest; the same 256 with the end-of-word mark;
one id per merge in file order (the first 48894 after the header line); <start_of_text>, <end_of_text>.
"""
import gzip
import html
import os
import re

CONTEXT_LENGTH = 77
N_MERGES = 49152 - 256 - 2
_EOW = "</w>"
_SPLIT = re.compile(r"'s|'t|'re|'ve|'m|'ll|'d|[a-z]+|[0-9]|[^\sa-z0-9]+")


def _byte_symbols():
    """the printable stand-in of every byte value, in id order"""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    rest = [b for b in range(256) if b not in keep]
    return {b: chr(b) for b in keep} | {b: chr(256 + i) for i, b in enumerate(rest)}, keep + rest


def bpe_file(bpe_path=None):
    path = bpe_path or os.environ.get("CLHIP_CLIP_BPE")
    if not path:
        raise FileNotFoundError("the CLIP tokenizer needs OpenAI's merges file bpe_simple_vocab_16e6.txt.gz, which is not part of this repository: pass "
                                "bpe_path or set $CLHIP_CLIP_BPE (or give the classifier pre-tokenized class_tokens)")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"CLIP merges file {path!r} not found (bpe_path / $CLHIP_CLIP_BPE); it is the user's to supply")
    return path


def clean(text):
    """what reaches the word split: unescaped, whitespace runs to one blank, lower case.  Needs no merges file; text that is not ASCII is refused here"""
    text = html.unescape(html.unescape(text)).strip()
    if not text.isascii():
        raise ValueError(f"class name {text!r} is not ASCII: the reference repairs such text with ftfy, which this tokenizer does without")
    return re.sub(r"\s+", " ", text).strip().lower()


class ClipTokenizer:
    def __init__(self, bpe_path=None):
        path = bpe_file(bpe_path)
        opener = gzip.open if path.endswith(".gz") else open
        with opener(path, "rb") as f:
            lines = f.read().decode("utf-8").split("\n")
        pairs = [tuple(l.split()) for l in lines[1:1 + N_MERGES]]
        if len(pairs) != N_MERGES or any(len(p) != 2 for p in pairs):
            raise ValueError(f"{path!r} does not hold {N_MERGES} merges after its header line")
        self.symbol, order = _byte_symbols()
        names = [self.symbol[b] for b in order]
        names = names + [n + _EOW for n in names] + [a + b for a, b in pairs] + ["<start_of_text>", "<end_of_text>"]
        self.ids = {n: i for i, n in enumerate(names)}
        self.rank = {p: i for i, p in enumerate(pairs)}
        self.sot, self.eot = self.ids["<start_of_text>"], self.ids["<end_of_text>"]
        self.vocab_size = len(names)
        self._done = {}

    def _merge(self, word):
        """the pieces of one word (its last symbol carries the end-of-word mark) after every applicable merge, lowest rank first"""
        if word in self._done:
            return self._done[word]
        parts = list(word[:-1]) + [word[-1] + _EOW]
        while len(parts) > 1:
            best = min(range(len(parts) - 1), key=lambda i: self.rank.get((parts[i], parts[i + 1]), N_MERGES))
            pair = (parts[best], parts[best + 1])
            if pair not in self.rank:
                break
            out, i = [], 0
            while i < len(parts):                              # every occurrence of the pair, left to right
                if i + 1 < len(parts) and (parts[i], parts[i + 1]) == pair:
                    out.append(parts[i] + parts[i + 1])
                    i += 2
                else:
                    out.append(parts[i])
                    i += 1
            parts = out
        self._done[word] = parts
        return parts

    def encode(self, text):
        out = []
        for word in _SPLIT.findall(clean(text)):
            out += [self.ids[p] for p in self._merge("".join(self.symbol[b] for b in word.encode("ascii")))]
        return out

    def __call__(self, texts, context_length=CONTEXT_LENGTH):
        """int64 [len(texts), context_length]; a row that is too long loses its tail, the end token included"""
        import torch
        texts = [texts] if isinstance(texts, str) else list(texts)
        out = torch.zeros(len(texts), context_length, dtype=torch.int64)
        for i, t in enumerate(texts):
            row = ([self.sot] + self.encode(t) + [self.eot])[:context_length]
            out[i, :len(row)] = torch.tensor(row, dtype=torch.int64)
        return out


_CACHE = {}


def tokenize(texts, context_length=CONTEXT_LENGTH, bpe_path=None):
    path = bpe_file(bpe_path)
    if path not in _CACHE:
        _CACHE[path] = ClipTokenizer(path)
    return _CACHE[path](texts, context_length)
