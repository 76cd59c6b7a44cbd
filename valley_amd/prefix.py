"""Conversation KV reuse: a session that keeps one sequence's KV cache across ``generate`` calls.

Every turn of a chat, and every further question about the same video, repeats the dialogue so far.  A ``PrefixSession``
remembers which tokens' K / V its cache holds; the next call computes only what follows the longest common prefix — 10-60 new
tokens instead of the tower and a 300-1800 token prefill.

    s = PrefixSession(model)
    s.prefill(prompt_ids, images)                      # optional: encode the video while the user is still typing
    out = model.generate(ids, images, prefix=s, ...)   # turn 1
    out = model.generate(ids2, images, prefix=s, ...)  # turn 2: only ids2's tail behind the common prefix is computed

``attention``: the kernel of a reused turn's 2..64 new tokens — "split" (ops.suffix_attention, the companion library
libvalley_hip_suffix.so) or "prefill" (ops.llama_attention, what a forward over a filled cache launches anyway).  Longer
suffixes, single tokens and a turn without a common prefix launch what they always launched.

One row, a 16-bit engine, no padding mask.  Not imported, and the library never loaded, unless a session is made."""
from __future__ import annotations

import os
from typing import List, Optional, Sequence

import torch

ATTENTION_ARMS = ("split", "prefill")
# the arm a session takes when neither the argument nor VALLEY_SUFFIX_ATTN names one: README "Conversation KV reuse" has the
# measurement (profiles/r13/prefix_ab.jsonl) behind it
DEFAULT_ATTENTION = "split"


def resolve_attention(value: Optional[str]) -> str:
    v = value if value is not None else (os.environ.get("VALLEY_SUFFIX_ATTN") or DEFAULT_ATTENTION)
    v = str(v).strip().lower()
    if v not in ATTENTION_ARMS:
        raise ValueError(f"attention must be one of {', '.join(repr(a) for a in ATTENTION_ARMS)} (VALLEY_SUFFIX_ATTN), got {value!r}")
    return v


def _clips(images) -> Optional[list]:
    if images is None:
        return None
    return list(images) if isinstance(images, (list, tuple)) else [images]


def _version(t) -> Optional[int]:
    try:
        return t._version
    except RuntimeError:                                     # an inference tensor tracks no version: contents decide
        return None


def same_frames(a, a_versions, b) -> bool:
    """The frames a cache was filled with against a new call's: the same tensor objects with unchanged ``_version``, or equal
    contents (one device comparison is cheaper than the tower)."""
    ca, cb = _clips(a), _clips(b)
    if ca is None or cb is None:
        return ca is None and cb is None
    if len(ca) != len(cb):
        return False
    for x, ver, y in zip(ca, a_versions, cb):
        if x is y and ver is not None and _version(x) == ver:
            continue
        if (x is y and ver is not None) or x.shape != y.shape or x.dtype != y.dtype or x.device != y.device or not torch.equal(x, y):
            return False                                     # (the same object, written since: its old contents are gone)
    return True


def common_prefix(cached_ids: Sequence[int], new_ids: Sequence[int], visual_ids, same_images: bool) -> int:
    """How many leading positions of ``new_ids`` a cache holding ``cached_ids`` already has: the longest common prefix, capped
    at len(new_ids) - 1 (one position must be computed to have logits); 0 when the frames differ, and 0 when a visual
    placeholder lies behind it (a reused turn never needs the tower).  Pure host logic."""
    if not same_images or not len(new_ids):
        return 0
    n = min(len(cached_ids), len(new_ids) - 1)
    p = 0
    while p < n and int(cached_ids[p]) == int(new_ids[p]):
        p += 1
    vis = {int(v) for v in visual_ids}
    if vis and any(int(t) in vis for t in new_ids[p:]):
        return 0
    return p


def _visual_ids(model) -> List[int]:
    tower = getattr(model.get_model(), "vision_tower", None)
    vc = getattr(tower, "config", None)
    names = ("im_patch_token", "im_start_token", "im_end_token", "vi_frame_token", "vi_start_token", "vi_end_token")
    return [int(getattr(vc, n)) for n in names if getattr(vc, n, None) is not None]


class PrefixSession:
    def __init__(self, model, attention: Optional[str] = None, initial_ctx: Optional[int] = None):
        if model.get_model().precision == "fp32":
            raise ValueError("PrefixSession needs a 16-bit engine: the fp32 validation engine keeps its own cache type")
        self.model = model
        self.attention = resolve_attention(attention)
        self.initial_ctx = initial_ctx                       # positions of the first allocation (default: the prompt + 256)
        self.limit = int(getattr(model.config, "max_position_embeddings", 2048))
        self.cache = None                                    # one row, growable up to ``limit``
        self.ids: List[int] = []                             # exactly the tokens whose K / V occupy rows [0, len(ids))
        self.frames, self._versions = None, ()
        self.stats = {"turns": 0, "reused": 0, "prefilled": 0, "tower_runs": 0}

    def reset(self) -> None:
        """Empty the session (another video): the cache's memory is kept, nothing in it is visible."""
        if self.cache is not None:
            self.cache.truncate(0)
        self.ids, self.frames, self._versions = [], None, ()

    @staticmethod
    def refuse(input_ids, attention_mask, precision: str, who: str = "PrefixSession.prefill") -> None:
        """What a session does not take, raised before anything is launched."""
        if input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ValueError(f"{who}: a prefix session holds one sequence, got input_ids {tuple(input_ids.shape)}")
        if input_ids.shape[1] < 1:
            raise ValueError(f"{who}: empty input_ids")
        if attention_mask is not None and bool((torch.as_tensor(attention_mask) == 0).any()):
            raise ValueError(f"{who}: an attention_mask with zeros (padding) is not supported with a prefix session")
        if precision == "fp32":
            raise ValueError(f"{who}: a prefix session needs a 16-bit engine (precision fp32)")

    def prefill(self, input_ids, images=None, attention_mask=None):
        """Bring the cache to ``input_ids`` [1, S]: keep the longest common prefix P with what it holds, run the forward over
        ``input_ids[:, P:]`` behind it (at P = 0 the ordinary forward, with the tower) and return the last position's
        logits, fp32 [1, V]."""
        self.refuse(input_ids, attention_mask, self.model.get_model().precision)
        return self.forward(input_ids, images).logits[:, -1, :]

    def forward(self, input_ids, images=None):
        """``prefill``'s work -> the model's output over the computed positions ``input_ids[:, P:]`` (``generate`` takes its last
        logits and the cache)."""
        from .llama import HipKVCache
        model = self.model
        input_ids = input_ids.to(model.device)
        new = [int(t) for t in input_ids[0].tolist()]
        S = len(new)
        if S > self.limit:
            raise ValueError(f"PrefixSession: {S} tokens exceed max_position_embeddings = {self.limit}")
        same = same_frames(self.frames, self._versions, images) if self.ids else False
        P = common_prefix(self.ids, new, _visual_ids(model), same)
        if self.cache is None:
            ctx = self.initial_ctx if self.initial_ctx is not None else (S + 256 + 127) // 128 * 128
            self.cache = model.get_model().llama.new_cache(1, max(S, min(self.limit, ctx)))
            self.cache.growable, self.cache.limit = True, self.limit
        assert isinstance(self.cache, HipKVCache)
        self.cache.truncate(min(P, self.cache.seq_len))
        self.ids = self.ids[:P]                              # (what the cache holds if the forward below raises)
        split = self.attention == "split" and P > 0
        out = model.forward(input_ids=input_ids[:, P:] if P else input_ids, images=images if P == 0 else None,
                            past_key_values=self.cache, use_cache=True, **({"suffix_attention": True} if split else {}))
        self.ids = new
        if P == 0:
            clips = _clips(images)
            self.frames, self._versions = images, tuple(_version(c) for c in clips) if clips else ()
            self.stats["tower_runs"] += int(images is not None)
        self.stats["turns"] += 1
        self.stats["reused"] += P
        self.stats["prefilled"] += S - P
        return out

    def reserve(self, n: int) -> None:
        """Room for ``n`` positions (``generate``: the prompt and the new tokens, capped at the model's limit)."""
        self.cache.reserve(min(self.limit, int(n)))

    def settle(self, sequence) -> None:
        """After a generation: ``ids`` = the first n tokens of the returned sequence, n = min(cache.seq_len, its length), and the
        cache truncated to n — a speculative step may have stored rows behind the stop."""
        seq = [int(t) for t in sequence.view(-1).tolist()]
        n = min(self.cache.seq_len, len(seq))
        self.cache.truncate(n)
        self.ids = seq[:n]
