"""Per-video scoring harness: the build's counterpart of the reference's offline loops
(prep.py:181-216, test2_prep.py:146-193,252-296,352-396,464-512): frames -> batched A-DISTS + DISTS
-> per-video columns -> CSV.  Host-side glue only; the scores come from the HIP modules.

Column arithmetic follows the reference to the type: the per-frame scores are the float32 arrays
the modules return (`.detach().cpu().numpy()`, test2_prep.py:152-155), so np.mean / np.std /
np.min / np.max are taken IN float32 and return np.float32 (:158-165), and
`frame_bias = video_score - frame_scores` is a float32 array (:167-168) serialised by `to_str`
(:123-125) as "['1.000000e-01', ...]".  `frame_count` is `len(frames_data)`, i.e. the number of
BATCHES of the DataLoader (:181), not of frames -- reproduced as written.
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional

import numpy as np
import torch

from . import prep, sharding

# column-name suffix per resize policy of test2_prep.py (:183-193, :286-296, :386-396, :502-509)
POLICY_SUFFIX = {None: "", "pil256_aspect": "", "full": "_full_size", "pil256": "_square",
                 "equal_pixels": "_pixel_count"}


def to_str(array) -> str:
    """test2_prep.py:123-125: the list of '{:.6e}' strings, as Python prints a list of str."""
    return str(["{:.6e}".format(num) for num in array])


def video_columns(name: str, frame_scores: np.ndarray, suffix: str = "") -> Dict[str, np.float32]:
    """The four per-video columns of one metric (prep.py:191-216, test2_prep.py:158-165,183-190):
    `name+suffix`, `..._std`, `..._min`, `..._max`, computed in the scores' own dtype (float32)."""
    s = np.asarray(frame_scores)
    if s.dtype != np.float32:
        s = s.astype(np.float32)
    base = name + suffix
    return {base: np.mean(s), f"{base}_std": np.std(s), f"{base}_min": np.min(s), f"{base}_max": np.max(s)}


def frame_bias(frame_scores: np.ndarray) -> np.ndarray:
    """test2_prep.py:167-168: video score (float32 mean) minus every frame's score."""
    s = np.asarray(frame_scores, dtype=np.float32)
    return np.mean(s) - s


def synthetic_frames(indices, h: int, w: int, device):
    """Frames `indices` of the synthetic video of BASELINE.json configs[3] / SURVEY.md 8d, generated ON THE DEVICE:
    frame i is a pure function of (i, h, w) -- the device generator is re-seeded with seed = frame index -- so any
    rank can produce any frame range without the video ever existing in host or device memory as a whole.
    Returns (ref, render) float32 (n,3,h,w): ref = U[0,1), render = clamp(ref + 0.1 N(0,1), 0, 1)."""
    idx = [int(i) for i in indices]
    ref = torch.empty(len(idx), 3, h, w, dtype=torch.float32, device=device)
    ren = torch.empty_like(ref)
    g = torch.Generator(device=device)
    for j, i in enumerate(idx):
        g.manual_seed(i)
        ref[j].uniform_(0.0, 1.0, generator=g)
        ren[j].normal_(0.0, 0.1, generator=g)
    ren.add_(ref).clamp_(0.0, 1.0)
    return ref, ren


@torch.no_grad()
def score_video(ref: torch.Tensor, render: torch.Tensor, dists_model: Optional[torch.nn.Module] = None,
                adists_model: Optional[torch.nn.Module] = None, batch_size: int = 8, group=None,
                policy: Optional[str] = None, keep_aspect_ratio: bool = False, suffix: str = "",
                with_frame_bias: bool = True, return_frame_scores: bool = False,
                shared_pyramid: bool = False) -> Dict[str, object]:
    """Score one video given as two (N,3,H,W) float32 tensors on the GPU, or -- with `policy` -- as two
    decoded uint8 (N,H,W,3) frame stacks on the GPU that are prepared per batch on the device
    (prep.prepare_frames: "interp256" = prep.py:89-95, "pil256" = prepare_image, ...).

    Frames are taken in batches of `batch_size` (test2_prep.py:120 uses 8); with torch.distributed
    initialised, frame ranges shard across ranks and the scores are all-gathered once (sharding.py).
    Argument order follows prep.py:186-189: model(ref, render); A-DISTS takes x = ref.
    Returns the reference's columns for this video: `A-DISTS`/`DISTS` (+`suffix`) with _std/_min/_max,
    and when `with_frame_bias` (test2_prep.py's first pass, suffix "") `frame_count`,
    `frame_bias_adists`, `frame_bias_dists`.

    shared_pyramid=True (both models required) scores every batch with pair.score_pair: the two metrics share one VGG
    pyramid instead of running it once each, frames given with a `policy` are prepared once per batch instead of once
    per metric, and a sharded video still costs one all-gather (of a two-column table).  The pair runs in A-DISTS'
    precision, a function of the frame size alone, so nothing has to be agreed between ranks.  The A-DISTS columns are
    those of the default mode bit for bit; the DISTS columns are those of DISTS(precision=<that precision>).
    """
    if ref.shape != render.shape:
        raise ValueError("ref and render differ in shape")
    if shared_pyramid and (dists_model is None or adists_model is None):
        raise ValueError("score_video(shared_pyramid=True) scores DISTS and A-DISTS from one pyramid: "
                         "pass both dists_model and adists_model")
    n = ref.shape[0]
    out: Dict[str, object] = {}

    def run(model_call: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], columns: int = 1) -> np.ndarray:
        def batch(lo, hi):
            a, b = ref[lo:hi], render[lo:hi]
            if policy is not None:
                a = prep.prepare_frames(a, policy, keep_aspect_ratio=keep_aspect_ratio)
                b = prep.prepare_frames(b, policy, keep_aspect_ratio=keep_aspect_ratio)
            return model_call(a, b)

        scores = sharding.score_frames_sharded(batch, n, batch_size, ref.device, group, columns)
        return scores.cpu().numpy()

    frames = {}
    if shared_pyramid:
        from .pair import score_pair

        def both(a, b):
            ds, ad = score_pair(dists_model, adists_model, a, b, batch_average=False, as_loss=False)
            return torch.stack([ad.reshape(-1).float(), ds.reshape(-1).float()], dim=1)

        table = run(both, columns=2)
        frames["A-DISTS"], frames["DISTS"] = np.ascontiguousarray(table[:, 0]), np.ascontiguousarray(table[:, 1])
    elif dists_model is not None and getattr(dists_model, "precision", None) == "auto" and policy is None:
        # one precision mode per video: under a process group rank 0's calibration verdict is broadcast BEFORE the
        # shards are scored (ranks whose shard is empty never enter forward(), so the collective cannot live there);
        # with no process group this is the plain precision_for.  (With `policy` the prepared size is only known per
        # batch; callers who shard prepared-on-the-fly videos call sharding.agree_precision with that size themselves.)
        sharding.agree_precision(dists_model, int(ref.shape[-2]), int(ref.shape[-1]), ref.device, group)
    if adists_model is not None and not shared_pyramid:
        frames["A-DISTS"] = run(lambda a, b: adists_model(a, b, as_loss=False))
    if "A-DISTS" in frames:
        out.update(video_columns("A-DISTS", frames["A-DISTS"], suffix))
    if dists_model is not None and not shared_pyramid:
        frames["DISTS"] = run(lambda a, b: dists_model(a, b, batch_average=False))
    if "DISTS" in frames:
        out.update(video_columns("DISTS", frames["DISTS"], suffix))
    if with_frame_bias:
        out["frame_count"] = -(-n // batch_size)  # len(DataLoader): batches, as the reference counts them
        if "A-DISTS" in frames:
            out["frame_bias_adists"] = to_str(frame_bias(frames["A-DISTS"]))
        if "DISTS" in frames:
            out["frame_bias_dists"] = to_str(frame_bias(frames["DISTS"]))
    if return_frame_scores:
        out["_frame_scores"] = frames
    return out


@torch.no_grad()
def score_videos(ref: torch.Tensor, renders, dists_model: torch.nn.Module, batch_size: int = 8, group=None,
                 policy: Optional[str] = None, keep_aspect_ratio: bool = False, suffix: str = "",
                 with_frame_bias: bool = True, return_frame_scores: bool = False, *,
                 adists_model: Optional[torch.nn.Module] = None, shared_pyramid: bool = False) -> List[Dict[str, object]]:
    """DISTS of K rendered videos of ONE scene against its reference video (the rows of the reference's tables that share
    a reference_folder, test2_prep.py:89,201,304,404): `ref` as score_video takes it, `renders` a (K,N,...) tensor or a
    list of K tensors of ref's shape.  Returns a list of K column dicts, entry k what
    score_video(ref, renders[k], dists_model, ...) returns -- but every batch of reference frames goes through the VGG
    pyramid ONCE for the K renders (DISTS.forward_group) instead of once per render.  Frames are taken in batches of
    `batch_size` reference frames (each with its K renders); under a process group the frame ranges shard as in
    score_video and ONE all-gather moves the (N, K) score table.

    adists_model (keyword only): each of the K dicts also carries the A-DISTS columns and `frame_bias_adists`, named and
    ordered as score_video(ref, renders[k], dists_model, adists_model, ...) returns them, from ADISTS.forward_group: the
    reference frames' pyramid, entropy weights and texture-probability chain run once per batch for the K renders.
    shared_pyramid=True (adists_model required): every batch is ONE pair.score_group call -- both metrics from one pyramid
    of the batch's references and renders, in A-DISTS' precision (score_video's shared_pyramid, for groups) -- and one
    all-gather moves the (N, 2K) table.  Without the two arguments the call is what it always was."""
    if shared_pyramid and adists_model is None:
        raise ValueError("score_videos(shared_pyramid=True) scores DISTS and A-DISTS from one pyramid: pass adists_model")
    rens = list(renders.unbind(0)) if torch.is_tensor(renders) else list(renders)
    if not rens:
        raise ValueError("score_videos: no renders")
    for k, t in enumerate(rens):
        if not torch.is_tensor(t) or t.shape != ref.shape:
            raise ValueError(f"score_videos: render {k} differs from ref in shape: {tuple(getattr(t, 'shape', ()))} vs "
                             f"{tuple(ref.shape)}")
    n, kk = ref.shape[0], len(rens)
    if not shared_pyramid and getattr(dists_model, "precision", None) == "auto" and policy is None:
        # one precision mode per video (score_video); the shared pyramid runs in A-DISTS' precision, a function of the size
        sharding.agree_precision(dists_model, int(ref.shape[-2]), int(ref.shape[-1]), ref.device, group)

    def run(call, columns):
        def batch(lo, hi):
            a, bs = ref[lo:hi], [t[lo:hi] for t in rens]
            if policy is not None:
                a = prep.prepare_frames(a, policy, keep_aspect_ratio=keep_aspect_ratio)
                bs = [prep.prepare_frames(b, policy, keep_aspect_ratio=keep_aspect_ratio) for b in bs]
            return call(a, torch.stack(bs, dim=1))

        scores = sharding.score_frames_sharded(batch, n, batch_size, ref.device, group, columns=columns)
        return scores.cpu().numpy().reshape(n, columns)

    tables = {}
    if shared_pyramid:
        from .pair import score_group

        def both(a, b):
            ds, ad = score_group(dists_model, adists_model, a, b)
            return torch.cat([ad.float(), ds.float()], dim=1)

        table = run(both, 2 * kk)
        tables["A-DISTS"], tables["DISTS"] = table[:, :kk], table[:, kk:]
    else:
        if adists_model is not None:
            tables["A-DISTS"] = run(lambda a, b: adists_model.forward_group(a, b, as_loss=False), kk)
        tables["DISTS"] = run(lambda a, b: dists_model.forward_group(a, b, batch_average=False), kk)
    outs = []
    for k in range(kk):
        frames = {name: np.ascontiguousarray(tables[name][:, k]) for name in ("A-DISTS", "DISTS") if name in tables}
        out: Dict[str, object] = {}
        for name, s in frames.items():  # (score_video's order: the A-DISTS columns first)
            out.update(video_columns(name, s, suffix))
        if with_frame_bias:
            out["frame_count"] = -(-n // batch_size)  # len(DataLoader): batches, as the reference counts them
            if "A-DISTS" in frames:
                out["frame_bias_adists"] = to_str(frame_bias(frames["A-DISTS"]))
            out["frame_bias_dists"] = to_str(frame_bias(frames["DISTS"]))
        if return_frame_scores:
            out["_frame_scores"] = frames
        outs.append(out)
    return outs


# the order test2_prep.py:183-193 assigns the first pass's columns in
COLUMN_ORDER = ("A-DISTS", "DISTS", "A-DISTS_std", "DISTS_std", "A-DISTS_min", "DISTS_min", "A-DISTS_max",
                "DISTS_max", "frame_count", "frame_bias_adists", "frame_bias_dists")


def add_video_columns(test_df, per_video: Iterable[Dict[str, object]], suffix: str = ""):
    """Assign the per-video results to the score table the way test2_prep.py:183-193 (and :286-296 etc. with a
    suffix) does: one new column per key, in the reference's order, each a list over the table's rows."""
    rows = list(per_video)
    if len(rows) != len(test_df):
        raise ValueError(f"{len(rows)} video results for a table of {len(test_df)} rows")
    order = [c if c.startswith("frame_") else c.replace("DISTS", "DISTS" + suffix, 1) for c in COLUMN_ORDER]
    for col in order:
        if rows and col in rows[0]:
            test_df[col] = [r[col] for r in rows]
    return test_df


def write_scores_csv(test_df, path: str) -> None:
    """test2_prep.py:512 / data_prep.py:120: `test_df.to_csv(path)` (index column included)."""
    test_df.to_csv(path)
