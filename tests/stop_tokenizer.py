"""Toy tokenizers for the stop-string tests: plain classes with what transformers' StopStringCriteria asks of a tokenizer
(``get_vocab``, ``__call__(text, add_special_tokens=False)``, ``_convert_id_to_token``, ``convert_tokens_to_string``) and what
the entry points ask (``batch_decode``).  No ``backend_tokenizer``: StopStringCriteria's matching mode is None (characters)."""
from types import SimpleNamespace

import torch

# about 27 pieces around '#': every way a token can start, end, cross or hold "###", the pieces of "stop", and the letters
# a-f (HF's vocabulary cleaning tokenizes the prefix "abcdef")
SMALL_PIECES = ("a", "b", "c", "d", "e", "f", "#", "##", "###", "####", "a#", "#b", "##c", "x###y", "st", "op", "stop", "s", "t",
                "o", "p", "x", "y", " ", "to", "p#", "#s")
ALPHABET = "abc#def"


class ToyTokenizer:
    def __init__(self, pieces):
        assert len(set(pieces)) == len(pieces)
        self.pieces = tuple(pieces)
        self.vocab = {p: i for i, p in enumerate(self.pieces)}
        self.longest = max(len(p) for p in self.pieces)

    def get_vocab(self):
        return dict(self.vocab)

    def encode(self, text):
        ids, i = [], 0
        while i < len(text):                                 # greedy longest match
            for n in range(min(self.longest, len(text) - i), 0, -1):
                if text[i:i + n] in self.vocab:
                    ids.append(self.vocab[text[i:i + n]])
                    i += n
                    break
            else:
                raise ValueError(f"no piece for {text[i:]!r}")
        return ids

    def __call__(self, text, add_special_tokens=False, **kw):
        if isinstance(text, (list, tuple)):
            return SimpleNamespace(input_ids=[self.encode(t) for t in text])
        return {"input_ids": self.encode(text)}

    def _convert_id_to_token(self, i):
        return self.pieces[int(i)]

    def convert_tokens_to_string(self, tokens):
        return "".join(tokens)

    def decode(self, ids, skip_special_tokens=True):
        ids = ids.tolist() if isinstance(ids, torch.Tensor) else ids
        return "".join(self.pieces[i] if 0 <= i < len(self.pieces) else "" for i in ids)

    def batch_decode(self, rows, skip_special_tokens=True):
        return [self.decode(r) for r in rows]


def small():
    return ToyTokenizer(SMALL_PIECES)


def piece_of(i: int) -> str:
    """Id i as 1-3 characters of ALPHABET: the digits of i in bijective base 7 (ids 0-6 are the letters themselves)."""
    n, out = i + 1, ""
    while n > 0:
        n, d = divmod(n - 1, len(ALPHABET))
        out = ALPHABET[d] + out
    return out


def generated(V: int = 306):
    """A vocabulary over a model's V ids (the golden model's 306): 7 + 49 + 250 pieces of one to three characters."""
    return ToyTokenizer([piece_of(i) for i in range(V)])
