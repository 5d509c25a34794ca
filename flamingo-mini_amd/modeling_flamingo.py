"""FlamingoModel drop-in (reference: flamingo_mini/modeling_flamingo.py).

Same public surface — FlamingoBaseModel / FlamingoGPT2 / FlamingoOPT / FlamingoModel, forward() arguments, freeze_*,
parameters_trainable(), state_dict_trainable(), prepare_inputs_for_generation(), generate_captions(),
score_sequences() — and the same parameter names, so `state_dict_trainable()` checkpoints interchange.
The frozen CLIP and GPT-2 / OPT backbones stay stock Hugging Face modules on PyTorch-ROCm; the perceiver
resampler and the gated cross-attention blocks hooked into the LM layer loop run in libflamingo_fusion.
"""
from __future__ import annotations

import contextlib
import logging
from abc import ABC, abstractmethod
from typing import Any, Dict, List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as TF
from transformers import PreTrainedModel
from transformers.modeling_outputs import CausalLMOutputWithPast

from . import decoding as D
from . import functional as F
from .backbones import load_language_model, load_vision_encoder
from .configuration_flamingo import FlamingoConfig
from .decoding import _DecodeSession, _beam_finalize, _repeat_leading      # noqa: F401  (importable from here, as before decoding.py)
from .gated_cross_attention import ModifiedLMBlock
from .perceiver_resampler import PerceiverResampler
from .utils import get_common_prefix_length


@contextlib.contextmanager
def suppress_model_loading_warnings(suppress: bool = True):
    logger = logging.getLogger("transformers.modeling_utils")
    level = logger.level
    if suppress:
        logger.setLevel(logging.CRITICAL)
    try:
        yield
    finally:
        logger.setLevel(level)


def _add_eoc_row(base_lm) -> None:
    """One extra embedding row for <EOC> (reference :315, :343: resize_token_embeddings(vocab_size + 1)).  from_pretrained builds the model
    on the meta device first (transformers >= 5); the mean / covariance initialisation of the new row cannot run there and is pointless
    (the checkpoint overwrites it), so it is only applied to real tensors."""
    real = base_lm.get_input_embeddings().weight.device.type != "meta"
    base_lm.resize_token_embeddings(base_lm.config.vocab_size + 1, mean_resizing=real)


class FlamingoBaseModel(ABC, PreTrainedModel):
    """CLIP -> PerceiverResampler -> LM whose layers were wrapped by ModifiedLMBlock (reference :43-306)."""

    config_class = FlamingoConfig
    _supports_sdpa = True
    lm_family: Optional[str] = None       # "gpt2" / "opt" on the subclasses the fixed-shape decode sessions know (decoding.py)

    def __init__(self, config: FlamingoConfig, suppress_warnings: bool = True):
        assert isinstance(config, FlamingoConfig)
        super().__init__(config)
        with suppress_model_loading_warnings(suppress_warnings):
            self.vision_encoder = load_vision_encoder(config)
        self.resampler = PerceiverResampler(
            dim=config.dim_visual, depth=config.resampler_depth, dim_head=config.resampler_dim_head,
            heads=config.resampler_heads, num_latents=config.resampler_num_latents,
            num_time_embeds=config.resampler_num_time_embeds, ff_mult=config.resampler_ff_mult, act=config.resampler_act)
        # Launch structure of the fusion path - plain attributes of the model (no environment variable), see set_launch_structure():
        # keys / values of all cross-attention layers in grouped launches ahead of the LM (functional.kv_project): 41.5 -> 40.2 ms per
        # step at the benchmark configuration; .hoist_kv = False restores the per-layer projection
        self.hoist_kv = True
        # 0: ONE projection call (one autograd node, one gradient bucket) for all layers; n > 0: one call per n consecutive layers, so that
        # under data parallelism the to_kv gradients of the upper layers are final - and their all-reduce starts - while backward is still
        # working on the lower ones (the data-parallel reducers set 4 = one grouped launch per call; a single bucket of all 36 to_kv
        # weights, 75 MB at flamingo-mini's size, would only become ready at the very end of backward)
        self.kv_project_group = 0

    def set_launch_structure(self, *, hoist_kv: Optional[bool] = None, kv_project_group: Optional[int] = None,
                             defer_wgrad: Optional[bool] = None, wgrad_group: "Optional[int] | str" = "keep") -> Dict[str, Any]:
        """How the fusion path batches its launches (results are identical for every setting; only the launch / gradient-bucket structure
        changes).  hoist_kv / kv_project_group: see __init__.  defer_wgrad / wgrad_group: the blocks' weight gradients run as launches
        grouped over `wgrad_group` consecutive layers (None = the library default of 12; data-parallel reducers use 4 so that a gradient
        bucket becomes final every four layers of backward).  Returns the PREVIOUS settings as a dict that can be passed back
        (`model.set_launch_structure(**previous)`) - data_parallel.GradientAllReducer.close() does exactly that."""
        blocks = [h.xattn_block for h in self.get_modified_layers()]
        prev = dict(hoist_kv=self.hoist_kv, kv_project_group=self.kv_project_group,
                    defer_wgrad=blocks[0].defer_wgrad if blocks else True, wgrad_group=blocks[0].wgrad_group if blocks else None)
        if hoist_kv is not None:
            self.hoist_kv = bool(hoist_kv)
        if kv_project_group is not None:
            self.kv_project_group = int(kv_project_group)
        for b in blocks:
            if defer_wgrad is not None:
                b.defer_wgrad = bool(defer_wgrad)
            if wgrad_group != "keep":
                b.wgrad_group = None if wgrad_group is None else int(wgrad_group)
        return prev

    def install_autograd_cuts(self, cuts, segment_layers: int = 4) -> None:
        """graphs.PiecewiseGraphedTrainStep: make the visual features and the hidden state in front of every `segment_layers`-th gated
        layer cut points of the autograd graph (`cuts.cut`), so that backward runs - and is captured - segment by segment.  None removes them."""
        self._autograd_cuts = cuts
        seg = max(1, int(segment_layers))
        if cuts is not None:
            # a K / V projection call must not serve layers of two segments (its backward node would be entered by both): one call per
            # segment, or per whole fraction of one
            if not (self.kv_project_group > 0 and seg % self.kv_project_group == 0):
                self._kv_group_before_cuts = (self.kv_project_group, seg)
                self.kv_project_group = seg
        elif hasattr(self, "_kv_group_before_cuts"):
            before, set_to = self._kv_group_before_cuts
            if self.kv_project_group == set_to:     # still what the cuts set (a reducer's close() may have restored its own value meanwhile)
                self.kv_project_group = before
            del self._kv_group_before_cuts
        for i, hook in enumerate(self.get_modified_layers()):
            hook.autograd_cut = cuts.cut if (cuts is not None and i > 0 and i % max(1, segment_layers) == 0) else None
        # a resampler that runs layer by layer (data parallelism: one gradient bucket per layer) makes every layer its own backward segment
        self.resampler.autograd_cut = cuts.cut if (cuts is not None and getattr(self.resampler, "layerwise", False)) else None

    def _init_weights(self, module):  # backbones initialise themselves; fusion modules use torch defaults like the reference
        pass

    def _init_layers(self, lm_layers: nn.ModuleList):
        """Wrap every `xattn_every`-th LM layer in place (reference :76-94)."""
        c = self.config
        for i in range(0, len(lm_layers), c.xattn_every):
            lm_layers[i] = ModifiedLMBlock(
                lm_layers[i], dim=c.dim, dim_visual=c.dim_visual, dim_head=c.xattn_dim_head, heads=c.xattn_heads,
                ff_mult=c.xattn_ff_mult, act=c.xattn_act, n_visual=c.resampler_num_latents)

    @abstractmethod
    def get_modified_layers(self) -> List[ModifiedLMBlock]:
        raise NotImplementedError

    # ---- freezing / trainable views (reference :100-138) ----
    def freeze_vm(self):
        self.vision_encoder.requires_grad_(False)

    def freeze_lm(self):
        """Freeze the LM except the (tied) token embedding and the gated xattn blocks."""
        self.lm.requires_grad_(False)
        self.lm.get_input_embeddings().weight.requires_grad = True
        for hook in self.get_modified_layers():
            hook.xattn_block.requires_grad_(True)

    def unfreeze_lm(self):
        self.lm.requires_grad_(True)

    def state_dict_trainable(self) -> Dict[str, torch.Tensor]:
        names = {n for n, p in self.named_parameters() if p.requires_grad}
        return {k: v for k, v in self.state_dict().items() if k in names}

    def parameters_trainable(self):
        return (p for p in self.parameters() if p.requires_grad)

    # ---- vision side (reference :140-181) ----
    def encode_resample_visuals(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """(N c h w) | (b N c h w) | (b N T c h w)  ->  (b N q d)."""
        if pixel_values.ndim == 4:
            b, N, T = 1, pixel_values.size(0), 1
        elif pixel_values.ndim == 5:
            b, N, T = pixel_values.size(0), pixel_values.size(1), 1
        elif pixel_values.ndim == 6:
            b, N, T = pixel_values.shape[:3]
        else:
            raise ValueError("pixel_values must have ndim 5 or 6!")
        frames = pixel_values.reshape(b * N * T, *pixel_values.shape[-3:])
        with torch.no_grad():
            feats = self.vision_encoder(frames).last_hidden_state                  # ((b N T), v, d), frozen
        feats = feats.reshape(b * N, T, feats.shape[-2], feats.shape[-1])          # frames go to the KV axis inside the resampler
        latents = self.resampler(feats)                                            # ((b N), q, d)
        return latents.reshape(b, N, latents.shape[-2], latents.shape[-1])

    # ---- forward (reference :183-306) ----
    def forward(self, input_ids=None, attention_mask=None, media_locations=None, pixel_values=None, visual_features=None,
                head_mask=None, inputs_embeds=None, use_cache: bool = False, past_key_values=None, return_dict: bool = True,
                labels=None, loss_reduction: str = "mean", text_time=None, label_smoothing: Optional[float] = None,
                z_loss: Optional[float] = None, output_last_hidden_state: bool = False, **kwargs) -> CausalLMOutputWithPast:
        """label_smoothing (eps in [0, 1]) and z_loss (zeta >= 0) regularise the loss, per scored token
            lse - (1 - eps) x_t - eps mean(x) + zeta lse^2           (functional.shifted_cross_entropy)
        None takes the optional config keys `label_smoothing` / `z_loss` (0 when absent), so loops that call model(**batch) - HF Trainer,
        GraphedTrainStep, PiecewiseGraphedTrainStep - pick them up from the config.  They are launch constants: a captured step keeps the
        values it was captured with.  The loss is the same in eval(): pass label_smoothing=0.0, z_loss=0.0 for the plain evaluation loss.
        output_last_hidden_state=True returns the lm_head's input as `hidden_states` = (last_hidden_state,) - what contrastive search compares;
        without it the output is what it always was."""
        assert return_dict, "can only use return_dict=True at the moment!"
        eps, zeta = F.check_loss_regularisers(getattr(self.config, "label_smoothing", 0.0) if label_smoothing is None else label_smoothing,
                                              getattr(self.config, "z_loss", 0.0) if z_loss is None else z_loss)
        assert (input_ids is None) != (inputs_embeds is None), "you must pass either input_ids or inputs_embeds!"
        ref = input_ids if input_ids is not None else inputs_embeds
        batch_size, seq_length = ref.shape[:2]
        device = ref.device
        xattn_past = None if past_key_values is None else past_key_values[0]
        lm_past = None if past_key_values is None else past_key_values[1]

        if visual_features is None:
            if xattn_past is None and pixel_values is not None:
                assert pixel_values.size(0) == batch_size, "pixel_values must have the same batch size as the textual input!"
                visual_features = self.encode_resample_visuals(pixel_values)
            else:  # cached K/V make the features irrelevant; only the shape is used
                visual_features = torch.zeros((batch_size, 1, self.config.resampler_num_latents, self.config.dim_visual),
                                              dtype=self.resampler.latents.dtype, device=device)
        if self.training and (getattr(self.lm, "gradient_checkpointing", False) or any(getattr(m, "gradient_checkpointing", False) for m in self.lm.modules())):
            # The conditioning of the hooks (and the K / V projected up front for every layer) lives for ONE call and is dropped when the LM
            # returns; a recomputation of LM blocks during backward would re-enter the hooks without it.
            raise NotImplementedError("activation checkpointing of the language model is not supported by the fused cross-attention hooks: "
                                      "their conditioning (visual features, hoisted K / V) is released when forward() returns. "
                                      "Disable gradient checkpointing (the frozen LM keeps few activations: only the trainable blocks save theirs).")
        if self.training and device.type == "cuda" and not torch.cuda.is_current_stream_capturing():
            # whatever optimizer drives an eager training loop: the error word of the fused cross-attention kernels' in-launch hand-offs is looked
            # at once per forward (non-blocking: the value the previous call copied to pinned memory) - raises SyncExchangeTimeout
            F.poll_sync_exchange("FlamingoBaseModel.forward")
        cuts = getattr(self, "_autograd_cuts", None)
        if cuts is not None and xattn_past is None:
            visual_features = cuts.cut(visual_features)      # (PiecewiseGraphedTrainStep: the resampler's backward becomes its own segment)
        if text_time is None:
            if media_locations is None:
                media_locations = torch.zeros((batch_size, seq_length), dtype=torch.int, device=device)
            text_time = F.text_time(media_locations)   # once per step, shared by every block (the reference recomputes it per layer)
        # (text_time given: a decode step of the static-cache path - generated tokens are never media tags, so the (b, 1) value of the
        # prompt's last token is valid for every later position and no per-step cumsum over a growing tensor is needed)
        hooks = self.get_modified_layers()
        hoisted = None
        if xattn_past is None and self.hoist_kv:
            # every layer's to_kv sees the same visual features: project for all layers in grouped launches (functional.kv_project)
            weights = [h.xattn_block.attn.to_kv.weight for h in hooks]
            cdt = F.autocast_compute_dtype(visual_features)
            if cdt is not None:              # torch.autocast over fp32 parameters: casts in the kernels' dtype (functional.autocast_compute_dtype)
                weights = F.autocast_params(weights, cdt)
            vf_cast = visual_features.to(weights[0].dtype)
            step = self.kv_project_group if self.kv_project_group > 0 else len(weights)
            hoisted = [kv for g in range(0, len(weights), step) for kv in F.kv_project(vf_cast, weights[g:g + step])]
        for i, hook in enumerate(hooks):
            hook.condition(visual_features, media_locations, None if xattn_past is None else xattn_past[i], text_time=text_time,
                           hoisted_kv=None if hoisted is None else hoisted[i])

        lm_kwargs = dict(input_ids=input_ids, attention_mask=attention_mask, inputs_embeds=inputs_embeds, use_cache=use_cache,
                         past_key_values=lm_past, return_dict=True, **kwargs)
        if head_mask is not None:
            lm_kwargs["head_mask"] = head_mask
        try:
            out = self.lm(**lm_kwargs)
        finally:
            # The conditioning is per call: dropping it here releases the hoisted K / V of every layer and - more importantly - the autograd
            # graph behind them.  The reference leaves it on the hooks until the next call; a graph kept alive that way pins the parameters'
            # AccumulateGrad nodes to the stream of THIS forward, which breaks a later capture of the step on another stream (graphs.py).
            for hook in hooks:
                hook.condition(None, None)
        logits = self.lm_head(out.last_hidden_state)

        new_xattn_past = [hook.kv_output for hook in hooks] if use_cache else None
        for hook in hooks:
            hook.kv_output = None

        loss = None
        if labels is not None:   # tokens < n predict n (reference :288-298)
            if logits.is_cuda and logits.dtype in (torch.float32, torch.bfloat16) and logits.ndim == 3 and seq_length > 1:
                loss = F.shifted_cross_entropy(logits, labels, reduction=loss_reduction, label_smoothing=eps, z_loss=zeta)      # two fused passes over the logits
            else:   # host-side / exotic dtypes: the stock op (the loss is not part of the accelerated fusion path)
                flat = logits[..., :-1, :].contiguous().view(-1, logits.size(-1))
                if flat.dtype in (torch.bfloat16, torch.float16):
                    flat = flat.float()
                target = labels[..., 1:].contiguous().view(-1)
                if eps == 0.0 and zeta == 0.0:
                    loss = TF.cross_entropy(flat, target, reduction=loss_reduction)
                else:   # the same definition as the fused path: the z term per scored token, under the same reduction
                    rows = TF.cross_entropy(flat, target, reduction="none", label_smoothing=eps)
                    if zeta != 0.0:
                        rows = rows + torch.where(target != -100, zeta * torch.logsumexp(flat, dim=-1).square(), torch.zeros_like(rows))
                    if loss_reduction == "none":
                        loss = rows
                    elif loss_reduction == "sum":
                        loss = rows.sum()
                    elif loss_reduction == "mean":
                        loss = rows.sum() / (target != -100).sum()
                    else:
                        raise ValueError(f"unknown reduction {loss_reduction}")

        return CausalLMOutputWithPast(
            loss=loss, logits=logits,
            past_key_values=(tuple(new_xattn_past), out.past_key_values) if use_cache else None,
            hidden_states=(out.last_hidden_state,) if output_last_hidden_state else getattr(out, "hidden_states", None), attentions=getattr(out, "attentions", None))


class FlamingoGPT2(FlamingoBaseModel):
    # GPT2LMHeadModel ties lm_head to the token embedding; declared here so that save_pretrained (safetensors: no aliased tensors) writes the
    # embedding once and from_pretrained re-ties it (transformers >= 5 refuses to save undeclared shared tensors)
    _tied_weights_keys = {"lm_head.weight": "lm.wte.weight"}
    lm_family = "gpt2"

    def __init__(self, config: FlamingoConfig):
        assert config.lm.startswith("gpt")
        super().__init__(config)
        base_lm = load_language_model(config)
        assert config.dim == base_lm.config.n_embd, \
            f"specified {config.dim=} in FlamingoConfig, but {config.lm} has hidden size={base_lm.config.n_embd}"
        _add_eoc_row(base_lm)
        self.lm = base_lm.transformer
        self.lm_head = base_lm.lm_head
        self._init_layers(self.lm.h)
        self.post_init()

    def get_modified_layers(self):
        return [layer for layer in self.lm.h if isinstance(layer, ModifiedLMBlock)]


class FlamingoOPT(FlamingoBaseModel):
    _tied_weights_keys = {"lm_head.weight": "lm.decoder.embed_tokens.weight"}
    lm_family = "opt"

    def __init__(self, config: FlamingoConfig):
        assert config.lm.startswith("facebook/opt")
        super().__init__(config)
        base_lm = load_language_model(config)
        assert config.dim == base_lm.config.hidden_size, \
            f"specified {config.dim=} in FlamingoConfig, but {config.lm} has hidden size={base_lm.config.hidden_size}"
        _add_eoc_row(base_lm)
        self.lm = base_lm.model
        self.lm_head = base_lm.lm_head
        self._init_layers(self.lm.decoder.layers)
        self.post_init()

    def get_modified_layers(self):
        return [layer for layer in self.lm.decoder.layers if isinstance(layer, ModifiedLMBlock)]


class FlamingoModel(PreTrainedModel):
    """LM-independent wrapper (reference :359-712)."""

    config_class = FlamingoConfig
    _LANGUAGE_MODEL_VERSIONS = {"gpt2": FlamingoGPT2, "facebook/opt": FlamingoOPT}
    # greedy decoding on the GPU (GPT-2- and, since round 5, OPT-backed models): fixed-shape decode steps (static_decode), replayed from a HIP graph (decode_graph);
    # plain attributes, settable per model - no environment variable
    static_decode = True
    decode_graph = True
    _keys_to_ignore_on_load_missing = [r"flamingo.vision_encoder"]

    def __init__(self, config: FlamingoConfig, model_class: Optional[type] = None):
        super().__init__(config)
        if model_class is None:
            model_class = self._find_flamingo_class(config.lm)
        self.flamingo: FlamingoBaseModel = model_class(config)
        if config.freeze_language_model:
            self.freeze_lm()
        if config.freeze_vision_model:
            self.freeze_vm()
        self.post_init()      # (transformers bookkeeping: the tied-weight table save_pretrained / from_pretrained use; _init_weights is a no-op)

    def _init_weights(self, module):
        pass

    @classmethod
    def is_lm_supported(cls, lm_id: str) -> bool:
        return any(lm_id.startswith(prefix) for prefix in cls._LANGUAGE_MODEL_VERSIONS)

    @classmethod
    def _find_flamingo_class(cls, language_model_id: str):
        for prefix, flamingo_class in cls._LANGUAGE_MODEL_VERSIONS.items():
            if language_model_id.startswith(prefix):
                return flamingo_class
        raise ValueError(f"unsupported language model {language_model_id}")

    def parameters_trainable(self):
        return self.flamingo.parameters_trainable()

    def install_autograd_cuts(self, cuts, segment_layers: int = 4) -> None:
        self.flamingo.install_autograd_cuts(cuts, segment_layers)

    def set_launch_structure(self, **kw):
        return self.flamingo.set_launch_structure(**kw)

    def freeze_vm(self):
        self.flamingo.freeze_vm()

    def freeze_lm(self):
        self.flamingo.freeze_lm()

    def unfreeze_lm(self):
        self.flamingo.unfreeze_lm()

    def state_dict_trainable(self):
        return self.flamingo.state_dict_trainable()

    def forward(self, input_ids=None, attention_mask=None, media_locations=None, pixel_values=None, visual_features=None,
                head_mask=None, inputs_embeds=None, use_cache: bool = False, past_key_values=None, return_dict: bool = True,
                labels=None, loss_reduction: str = "mean", label_smoothing: Optional[float] = None, z_loss: Optional[float] = None,
                **kwargs) -> CausalLMOutputWithPast:
        """label_smoothing / z_loss: see FlamingoBaseModel.forward (None = the config's optional keys, 0 when absent)."""
        return self.flamingo(label_smoothing=label_smoothing, z_loss=z_loss,input_ids=input_ids, attention_mask=attention_mask, media_locations=media_locations,
                             pixel_values=pixel_values, visual_features=visual_features, head_mask=head_mask,
                             inputs_embeds=inputs_embeds, use_cache=use_cache, past_key_values=past_key_values,
                             return_dict=return_dict, labels=labels, loss_reduction=loss_reduction, **kwargs)

    # ---- generation helpers (reference :464-605) ----
    def prepare_inputs_for_generation(self, input_ids, media_locations=None, attention_mask=None, pixel_values=None,
                                      visual_features=None, past=None, past_key_values=None, **kwargs) -> Dict[str, Any]:
        """Replicate visuals / media_locations to the beam-expanded batch; with a cache only the last token is fed."""
        n_inputs = input_ids.shape[0]

        def expand(t):
            if t is None or t.shape[0] == n_inputs:
                return t
            assert n_inputs % t.shape[0] == 0
            return _repeat_leading(t, n_inputs // t.shape[0])

        cache = past_key_values if past_key_values is not None else past
        if cache is not None:
            input_ids = input_ids[:, -1:]
        return dict(input_ids=input_ids, past_key_values=cache, media_locations=expand(media_locations),
                    attention_mask=attention_mask, pixel_values=expand(pixel_values), visual_features=expand(visual_features), **kwargs)

    def _reorder_cache(self, past, beam_idx):
        xattn_past, lm_past = past
        pick = lambda t: t.index_select(0, beam_idx.to(t.device))
        xattn_new = tuple(tuple(pick(t) for t in layer) for layer in xattn_past)
        if hasattr(lm_past, "reorder_cache"):      # transformers >= 4.36 Cache objects
            lm_past.reorder_cache(beam_idx)
            lm_new = lm_past
        else:
            lm_new = tuple(tuple(pick(t) for t in layer) for layer in lm_past)
        return xattn_new, lm_new

    @torch.no_grad()
    def greedy_generate(self, input_ids, media_locations, attention_mask, pixel_values=None, visual_features=None,
                        max_length: int = 150, eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None):
        """Cached greedy decoding (the caption tokens/sec path); see generate()."""
        return self.generate(input_ids, media_locations=media_locations, attention_mask=attention_mask, pixel_values=pixel_values,
                             visual_features=visual_features, max_length=max_length, eos_token_id=eos_token_id, pad_token_id=pad_token_id)

    def _decode_step(self, step_ids, ml, am, past, pixel_values, visual_features):
        out = self.flamingo(input_ids=step_ids, attention_mask=am, media_locations=ml, use_cache=True, past_key_values=past,
                            pixel_values=pixel_values if past is None else None, visual_features=visual_features if past is None else None)
        return out.logits[:, -1].float(), out.past_key_values

    def _score_step(self, step_ids, ml, am, past, pixel_values, visual_features):
        """_decode_step for score_candidates: the last position's logits as a VIEW in the model's dtype (no .float() copy) - what
        functional.logprob_gather reads in place through the row stride."""
        out = self.flamingo(input_ids=step_ids, attention_mask=am, media_locations=ml, use_cache=True, past_key_values=past,
                            pixel_values=pixel_values if past is None else None, visual_features=visual_features if past is None else None)
        return out.logits[:, -1], out.past_key_values

    def _contrastive_step(self, step_ids, ml, am, past, pixel_values, visual_features):
        """_decode_step for contrastive search: also the lm_head's input of every position fed, (rows, positions, dim) in the model's dtype."""
        out = self.flamingo(input_ids=step_ids, attention_mask=am, media_locations=ml, use_cache=True, past_key_values=past, output_last_hidden_state=True,
                            pixel_values=pixel_values if past is None else None, visual_features=visual_features if past is None else None)
        return out.logits[:, -1].float(), out.hidden_states[-1], out.past_key_values

    _filter_logits = staticmethod(D.filter_logits)         # the torch restatements the dynamic loops use
    _process_logits = staticmethod(D.process_logits)

    @torch.no_grad()
    def generate(self, inputs=None, media_locations=None, attention_mask=None, pixel_values=None, visual_features=None,
                 max_length: int = 150, num_beams: int = 1, do_sample: bool = False, temperature: float = 1.0, top_k: int = 0,
                 top_p: float = 1.0, eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None, bos_token_id: Optional[int] = None,
                 early_stopping: bool = True, length_penalty: float = 1.0, use_cache: bool = True, generator: Optional[torch.Generator] = None,
                 input_ids=None, static_decode: Optional[bool] = None, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                 min_length: int = 0, min_new_tokens: int = 0, return_dict_in_generate: bool = False, output_logprobs: bool = False,
                 num_return_sequences: int = 1, candidate_ids=None, bad_words_ids=None, num_beam_groups: int = 1,
                 diversity_penalty: float = 0.0, guidance_scale: float = 1.0, min_p: float = 0.0, typical_p: float = 1.0,
                 epsilon_cutoff: float = 0.0, eta_cutoff: float = 0.0, penalty_alpha: float = 0.0, **unsupported):
        """Text generation with the cached cross-attention path: the first step runs CLIP + resampler and fills the xattn K/V and LM caches,
        every later step feeds one token (reference: HF `generate` through prepare_inputs_for_generation / _reorder_cache, :464-548).
        transformers >= 4.50 no longer gives PreTrainedModel a `generate`, so the decoding strategies the reference's callers use are
        implemented here: greedy, multinomial sampling (do_sample, temperature, top_k, top_p) and beam search (num_beams, length_penalty,
        early_stopping).  Unknown generation arguments raise instead of being ignored.
        The three steps are the argument checks, decoding.route - the one statement of which path a call takes - and the call itself.
        Sampling and beam search (num_beams <= 8) take the fixed-shape, graph-replayed path of greedy decoding (decoding._DecodeSession) only
        when `static_decode=True` is passed explicitly (GPU tensors, a GPT-2- or OPT-backed model, a prompt shorter than max_length - 1);
        otherwise they run the dynamic loops (decoding.dynamic_decode / beam_search), as they always have.  The two paths draw DIFFERENT token streams from the same seed: the static path draws by inverse CDF in
        vocabulary order from one uniform number per token (functional.sample_tokens), the dynamic loop with torch.multinomial.  Both are
        reproducible per seed (`generator`).
        Logits processors, as in transformers: `repetition_penalty` (1 = off), `no_repeat_ngram_size` (0 = off) and `min_length` /
        `min_new_tokens` (both need eos_token_id) act on the logits of every step BEFORE the selection of every mode, against the whole
        sequence so far, prompt included.  On the static path they are one in-place launch inside the replayed step
        (functional.process_logits; int64 ids, max_length <= 4096 - otherwise the dynamic loop runs), on the dynamic paths the torch
        restatement _process_logits.  They are offered for GPU tensors only: with CPU tensors generate() raises TypeError for them, as it
        did before they existed (the processor kernel has no CPU form; static_decode=True raises what ffi.require_cuda raises).  Deliberate deviation from transformers in beam search: the log-softmax is taken AFTER the processors, so
        the mass of banned tokens is renormalised over the rest, where transformers penalises log-probabilities without renormalising.
        Outputs: `return_dict_in_generate=True` returns a decoding.GenerateOutput (sequences, sequences_scores, token_logprobs) instead of
        the ids.  `output_logprobs=True` (greedy and sampling; needs return_dict_in_generate) fills token_logprobs, aligned with
        sequences[:, L0:]: the log-softmax, at the chosen token, of the step's logits as the selection sees them - after the logits
        processors, before temperature / top-k / top-p -, 0 at the pad positions of a row that had finished; and sequences_scores =
        sum(token_logprobs) / float32(len ** length_penalty), len counting the prompt and the generated tokens up to and including eos.
        On the static path they are float32 from one launch inside the replayed step (functional.token_logprobs, GPU tensors only; with
        static_decode=None CPU tensors take the dynamic loop); the dynamic loop takes torch's log_softmax in float32 (float64 for a float64
        model).  With beam search sequences_scores is the normalised score the search ranked by, and output_logprobs raises ValueError.
        `num_return_sequences=n`: sampling repeats every sequence n times (the visuals are encoded once per sequence), beam search (n <=
        num_beams) returns the n best of the hypotheses and open beams its tail ranks, best first, missing ones all pad with score -inf;
        output rows s * n + j.  Greedy decoding has one result: n > 1 raises ValueError.
        Constraints (lists of lists of token ids, the same for every row; ValueError for empty input, empty entries and ids outside the
        vocabulary): `candidate_ids` restricts what is generated to one of the candidates followed by eos - every step's logits keep only the
        tokens that continue a candidate along the row's own generated tokens, and eos where one ends (a candidate may be a prefix of
        another); it needs eos_token_id, cannot be combined with min_length / min_new_tokens, no candidate may contain eos, and prompt +
        longest candidate + eos must fit max_length.  `bad_words_ids` bans, as transformers does, the last token of a word whenever the
        sequence so far - prompt included - ends with the word's other tokens.  Both act after the logits processors and before the
        selection and token_logprobs of every mode, so log-probabilities and beam scores are renormalised over the allowed set: greedy or
        beam search under `candidate_ids` with output_logprobs / sequences_scores / num_return_sequences is closed-set classification with
        the probability of the chosen candidate(s).  On the static path they are one in-place launch inside the replayed step
        (functional.constrain_logits: int64 ids, max_length <= 4096, a vocabulary of at most 262144 - otherwise the dynamic loop runs) that
        reads the tables from device buffers, so a later call with other candidates of the same capacity class (sizes rounded up to powers
        of two) reuses the session and its captured graph; on the dynamic paths decoding.constrain_logits_torch, which - unlike the
        processors - also runs on CPU tensors.  Known and accepted: beam search with fewer candidates than beams and early_stopping=False
        never collects num_beams hypotheses, so it runs to max_length with dead beams (score -inf); the result is still the best
        candidates, on both paths.  The candidates are one set for the whole batch.
        Diverse beam search (Vijayakumar et al.): `num_beam_groups=G` (it must divide num_beams; not with do_sample) splits the beams into G
        groups of num_beams / G that are searched one after another inside every step, and `diversity_penalty` (>= 0, finite; it needs G > 1)
        is subtracted from a group's candidate once for every live beam of an earlier group that chose the same token in that step.  Every
        group keeps its own hypotheses and stops on its own; the result ranks the entries of all groups together, so
        num_return_sequences=n returns the n best across the groups.  The penalised score is the beam's running score, penalties
        accumulate over the steps as in the published algorithm: sequences_scores under groups are NOT pure log-probabilities.  The
        penalty is soft, so two groups may still return the same sequence.  G = 1 is plain beam search, call for call; G > 1 with penalty 0
        runs G independent searches of num_beams / G beams.  Routing is that of beam search: the static session (functional.group_beam_step
        inside the replayed step: the row pass of beam_step and one group walk, no host round trip) only with static_decode=True, otherwise
        the dynamic loop, which also runs on CPU tensors.
        Classifier-free guidance (transformers' `guidance_scale`; Kornblith et al., "Guiding image captioning models toward more specific
        captions") says how strongly the media count: every sequence is decoded twice, with its media and - the same ids, media_locations all
        zero, which leaves the frozen LM with the gated feed-forward: the model's own text prior - without, and every step selects from
            scores = log p(. | text) + guidance_scale * (log p(. | media, text) - log p(. | text)).
        1.0 is off (exactly the paths without it); any other finite value >= 0 turns it on: > 1 extrapolates away from the prior (captions say
        what is in THIS image), values in (0, 1) interpolate towards it, 0 is the prior alone.  Negative, non-finite and non-numeric values
        raise ValueError.  Guidance comes FIRST, as in transformers: the logits processors, the constraints, sampling, beam search, groups and
        the log-probabilities all act on the guided scores, so token_logprobs and sequences_scores are the log-softmax of the GUIDED scores
        - renormalised, not model probabilities.  num_return_sequences for sampling repeats the rows before they are doubled.  The LM runs
        on [conditional rows ; unconditional rows] (2 x the rows; the visuals are encoded once and repeated).  On the static path
        the combination is one launch inside the replayed step (functional.guided_logits) whose scale is a device scalar: calls with other
        scales reuse the session and its graph.  Routing: guided greedy decoding takes the static path by default on the GPU, guided sampling
        and beam search with static_decode=True; CPU tensors take the dynamic loops (decoding.guided_logits_torch), static_decode=True with
        CPU tensors raises what ffi.require_cuda raises.  A negative prompt (other ids for the unconditional branch) is not offered.
        Truncation samplers (with do_sample=True, not with beam search; ValueError otherwise and for values out of range), transformers'
        warpers with min_tokens_to_keep = 1, applied in transformers' order after temperature, top_k and top_p: `min_p` in [0, 1] (0 = off)
        keeps the tokens whose probability is at least min_p times the largest; `typical_p` in (0, 1] (1 = off) keeps the tokens whose
        information content is nearest the distribution's entropy until they hold typical_p of the mass (locally typical sampling);
        `epsilon_cutoff` in [0, 1) (0 = off) drops the tokens below that probability; `eta_cutoff` in [0, 1) (0 = off) drops those below
        min(eta, sqrt(eta) exp(-entropy)) (eta sampling).  Every rule acts on values, so equal logits stay or go together, and each keeps the
        largest.  The exact rules are those of ff_sample_token_truncated in include/flamingo_fusion.h.  Routing is that of sampling: the
        static session (the rules and the draw are one launch inside the replayed step, functional.sample_tokens; the values are launch
        constants and part of the session key) only with static_decode=True, otherwise the dynamic loop with
        decoding.truncate_logits_torch, which also runs on CPU tensors.  token_logprobs stay the log-softmax before temperature and every
        filter.  Not offered: min_tokens_to_keep > 1, per-row values, the four truncation samplers under beam sampling.
        Beam sampling (transformers' beam-sample): `do_sample=True` with `num_beams > 1` is beam search whose every step DRAWS its 2 *
        num_beams candidates instead of taking the best: temperature, top_k and top_p warp each beam's log-probabilities (nothing is
        renormalised, as in transformers), the beam's running score is added, and 2 * num_beams continuations are drawn without replacement
        from the softmax over the sequence's num_beams * vocab accumulated scores - a Gumbel top-k, the Plackett-Luce law of
        torch.multinomial(replacement=False) -; the drawn ones are sorted by accumulated score and walked as in beam search.  It returns
        several distinct, reasonably likely sequences, each with its score: num_return_sequences, sequences_scores, the processors,
        candidate_ids, bad_words_ids and guidance_scale compose as with beam search.  The exact rules are S1 - S6 of ff_beam_sample_step in
        include/flamingo_fusion.h.  Routing is that of beam search: the static session (functional.beam_sample_step inside the replayed
        step; the noise is a function of a per-call seed drawn from `generator`, the step's length, the row and the column, so no random
        tensor exists and eager and replayed steps agree; num_beams <= 8) only with static_decode=True, otherwise the dynamic loop
        (decoding.beam_sample_select_torch), which also runs on CPU tensors.  As with token sampling the two paths draw DIFFERENT streams
        from one seed; each is reproducible per `generator`.  Known and accepted: with top_k < 2 * num_beams the first step has fewer
        finite candidates than it draws and the missing beams are dead.  num_beam_groups > 1, min_p / typical_p / epsilon_cutoff /
        eta_cutoff and output_logprobs keep their ValueErrors under beam sampling.
        Contrastive search (Su et al. 2022, "A Contrastive Framework for Neural Text Generation"; transformers' `penalty_alpha` with `top_k`)
        is the deterministic answer to the repetitions of greedy and beam search: every step lists the `top_k` most probable next tokens,
        feeds EACH of them to the LM, and chooses the one that maximises
            (1 - penalty_alpha) * p(token) - penalty_alpha * max_j cos(h_token, h_j),
        h the lm_head's input and j the positions so far (the prompt's left padding excluded): confident, and unlike what was said.  0 is off
        (exactly the paths without it, call for call; `top_k` with greedy decoding stays ignored); it is on for 0 < penalty_alpha <= 1
        together with 2 <= top_k <= 8, do_sample=False and num_beams == 1.  ValueError: a non-finite or negative value or one above 1; a
        top_k outside that range while it is on; do_sample, num_beams > 1, num_beam_groups > 1, guidance_scale != 1, num_return_sequences > 1.
        The exact rules are T and C1 - C9 of include/flamingo_fusion.h: probabilities come from the log-softmax of the logits after the
        processors and constraints, ties go to the more probable candidate, a banned candidate (probability 0) never wins - in
        transformers it can, on its penalty alone - and the norms are clamped at 1e-12 where transformers divides by zero.  It composes with
        repetition_penalty, no_repeat_ngram_size, min_length / min_new_tokens, candidate_ids, bad_words_ids, eos / pad,
        return_dict_in_generate and output_logprobs: token_logprobs is the chosen candidate's log-probability, the log-softmax of the
        processed logits as for greedy decoding, and sequences_scores their length-normalised sum.  Routing is that of beam search: the
        static session (decoding._ContrastiveSession: the LM runs on batch * top_k rows; the ranking, the choice and the eos bookkeeping are
        one launch inside the replayed step, functional.contrastive_step, the candidates another, functional.topk_logprobs, and the LM
        cache follows the chosen row through functional.beam_gather; penalty_alpha is a device scalar, so calls with other values reuse the
        session and its graph, and top_k is part of the session key) only with static_decode=True, which needs GPU tensors; otherwise the
        dynamic loop (decoding.contrastive_search), which also runs on CPU tensors.  Not offered: guidance, top_k above 8, per-row
        penalty_alpha."""
        procs = D.check_generate_args(unsupported, use_cache, repetition_penalty, no_repeat_ngram_size, min_length, min_new_tokens, eos_token_id)
        n_ret = D.check_output_args(return_dict_in_generate, output_logprobs, num_return_sequences, num_beams, do_sample)
        groups = D.check_group_args(num_beam_groups, diversity_penalty, num_beams, do_sample)
        gkw = {} if groups is None else {"groups": groups}                   # nothing is passed on without groups: the calls are what they were
        guidance = D.check_guidance_args(guidance_scale)
        trunc = D.check_truncation_args(min_p, typical_p, epsilon_cutoff, eta_cutoff, do_sample, num_beams)
        tkw = {} if trunc is None else {"truncation": trunc}                 # nothing is passed on without them: the calls are what they were
        contr = D.check_contrastive_args(penalty_alpha, top_k, do_sample, num_beams, num_beam_groups, guidance_scale, n_ret)
        ids = inputs if inputs is not None else input_ids
        assert ids is not None and media_locations is not None, "generate() needs input ids and media_locations"
        cons = D.check_constraint_args(candidate_ids, bad_words_ids, self.flamingo.lm.config.vocab_size, eos_token_id, procs, ids.shape[1], max_length)
        ckw = {} if cons is None else {"constraints": cons}                   # nothing is passed on without constraints: the calls are what they were
        rkw = {} if cons is None else dict(constraints_on=True, vocab=self.flamingo.lm.config.vocab_size, table_entries=max(cons.caps()[1:]))
        am = attention_mask if attention_mask is not None else torch.ones_like(ids)
        ml = media_locations
        pad = pad_token_id if pad_token_id is not None else eos_token_id
        beam_sample = bool(do_sample) and num_beams > 1                      # a beam search whose selection draws: route() sees it as one
        if beam_sample and not (0 < temperature < float("inf") and top_k >= 0 and 0 < top_p <= 1):
            raise ValueError(f"generate(): beam sampling needs a positive, finite temperature, top_k >= 0 and top_p in (0, 1], got {temperature!r}, {top_k!r}, {top_p!r}")
        skw = dict(sampling=D.Sampling(float(temperature), int(top_k), float(top_p)), generator=generator) if beam_sample else {}
        path = D.route(is_cuda=ids.is_cuda, num_beams=num_beams, do_sample=do_sample and not beam_sample, static_decode=static_decode, model_default=self.static_decode, lm_family=self.flamingo.lm_family,
                       L0=ids.shape[1], max_length=max_length, ids_is_int64=ids.dtype == torch.long, procs_on=procs is not None, procs_given=procs.given() if procs is not None else (),
                       logprobs_on=bool(output_logprobs), **rkw, **({} if guidance is None else {"guidance_on": True}),
                       **({"beam_sample_on": True} if beam_sample else {}), **({} if contr is None else {"contrastive_on": True}))
        if n_ret > 1 and num_beams <= 1:                                     # sampling: every sequence n times, its visuals encoded once
            if visual_features is None and pixel_values is not None:
                visual_features, pixel_values = self.flamingo.encode_resample_visuals(pixel_values), None
            ids, ml, am = _repeat_leading(ids, n_ret), _repeat_leading(ml, n_ret), _repeat_leading(am, n_ret)
            if visual_features is not None:
                visual_features = _repeat_leading(visual_features, n_ret)
        step, reorder = self._decode_step, self._reorder_cache
        if guidance is not None:
            if visual_features is None and pixel_values is not None:         # encoded once; both halves of the LM batch carry the same features
                visual_features, pixel_values = self.flamingo.encode_resample_visuals(pixel_values), None
            if path == "static":
                gkw = dict(gkw, guidance=guidance)
            else:                                                            # the loops see a model whose logits are the guided scores
                step, reorder = D.guided_step(step, guidance), D.guided_reorder(reorder)
        n_beams_out = n_ret if num_beams > 1 and (return_dict_in_generate or n_ret > 1) else None      # None: the search's single result, as ever
        if contr is not None and path == "static":
            res = D._static_decode(self, ids, ml, am, pixel_values, visual_features, max_length, eos_token_id, pad, processors=procs, logprobs=bool(output_logprobs),
                                   contrastive=contr, **ckw)
        elif contr is not None:
            lp_dtype = (torch.float64 if next(self.parameters()).dtype == torch.float64 else torch.float32) if output_logprobs else None
            res = D.contrastive_search(self._contrastive_step, self._reorder_cache, ids, ml, am, pixel_values, visual_features, max_length, contr, eos_token_id, pad,
                                       processors=procs, logprob_dtype=lp_dtype, **ckw)
        elif path == "static":
            res = D._static_decode(self, ids, ml, am, pixel_values, visual_features, max_length, eos_token_id, pad, generator=generator, processors=procs,
                                   sampling=D.Sampling(float(temperature), int(top_k), float(top_p)) if do_sample else None,
                                   beams=D.Beams(int(num_beams), bool(early_stopping), float(length_penalty)) if num_beams > 1 else None,
                                   logprobs=bool(output_logprobs), n_return=n_beams_out, **ckw, **gkw, **tkw)
        elif num_beams > 1:
            res = self._beam_search(ids, ml, am, pixel_values, visual_features, max_length, num_beams, eos_token_id, pad, early_stopping, length_penalty, processors=procs,
                                    n_return=n_beams_out, **ckw, **gkw, **skw, **({} if guidance is None else {"step": step, "reorder_cache": reorder}))
        else:
            # the log-softmax is taken in float32, the dtype of the logits _decode_step hands the loop; a model that computes in float64 keeps
            # its precision (a float32 log-softmax would throw away what a float64 evaluation on the host is run for)
            lp_dtype = (torch.float64 if next(self.parameters()).dtype == torch.float64 else torch.float32) if output_logprobs else None
            res = D.dynamic_decode(step, ids, ml, am, pixel_values, visual_features, max_length, eos_token_id, pad,
                                   sampling=D.Sampling(temperature, top_k, top_p) if do_sample else None, generator=generator, processors=procs,
                                   logprob_dtype=lp_dtype, **ckw, **tkw)
        if not return_dict_in_generate:
            return res[0] if n_beams_out else res
        if n_beams_out:
            return D.GenerateOutput(sequences=res[0], sequences_scores=res[1])
        if output_logprobs:
            seqs, lps = res
            return D.GenerateOutput(sequences=seqs, token_logprobs=lps, sequences_scores=D.sequence_scores(seqs, lps, ids.shape[1], eos_token_id, float(length_penalty)))
        return D.GenerateOutput(sequences=res)

    @property
    def _decode_sessions(self) -> dict:
        return D._DECODE_SESSIONS.get(self, {})

    def reset_decode_sessions(self) -> None:
        D._DECODE_SESSIONS.pop(self, None)

    def _beam_search(self, ids, ml, am, pixel_values, visual_features, max_length, nb, eos, pad, early_stopping, length_penalty, processors=None, n_return=None,
                     step=None, reorder_cache=None, **constraints):
        """The dynamic beam search (decoding.beam_search) over this model's _decode_step / _reorder_cache; `constraints=`, `groups=` and
        `sampling=` / `generator=` (beam sampling) travel as keywords and only when given, and so do `step=` / `reorder_cache=`, the guided wrappers of the two (decoding.guided_step)."""
        return D.beam_search(step or self._decode_step, reorder_cache or self._reorder_cache, ids, ml, am, pixel_values, visual_features, max_length, nb, eos, pad, early_stopping, length_penalty, processors,
                             n_return=n_return, **constraints)

    @torch.no_grad()
    def generate_captions(self, processor, pixel_values=None, images=None, prompt: str = "<image>", max_length: int = 150,
                          num_beams: int = 1, device=None, return_scores: bool = False, candidates=None, bad_words=None, **kwargs):
        """Caption a batch of images; the prompt is replicated for every image (reference :550-605).  `kwargs` are generation
        arguments (do_sample, temperature, top_k, top_p, length_penalty, repetition_penalty, no_repeat_ngram_size, min_length,
        min_new_tokens, num_return_sequences, output_logprobs, return_dict_in_generate, num_beam_groups, diversity_penalty, guidance_scale,
        min_p, typical_p, epsilon_cutoff, eta_cutoff, penalty_alpha, ...) and go to
        generate(), which rejects unknown ones.  num_beams=4, num_beam_groups=4, diversity_penalty=1.0, num_return_sequences=4,
        return_scores=True gives the 4 best DIFFERENT captions of diverse beam search with the (penalised) scores they were ranked by.
        guidance_scale=1.5 weighs the image against the language model's prior (classifier-free guidance, see generate()).
        penalty_alpha=0.6, top_k=4 is contrastive search: deterministic captions that do not repeat themselves (see generate()).
        `return_scores=True` returns (captions, scores), the scores floats from GenerateOutput.sequences_scores (beam search: the score the
        search ranked by; greedy and sampling: the length-normalised sum of the token log-probabilities).  With num_return_sequences = n > 1
        the captions (and the scores) are a list of one list of n per image.
        `candidates` / `bad_words` (lists of strings) become generate()'s candidate_ids / bad_words_ids: every string is tokenised VERBATIM
        with processor.tokenizer(s, add_special_tokens=False) - a leading space is part of the string and the caller's business (after a
        prompt that ends in a word, BPE vocabularies spell the next word " cat", not "cat")."""
        for name, strings in (("candidate_ids", candidates), ("bad_words_ids", bad_words)):
            if strings is not None:
                if isinstance(strings, str):
                    raise ValueError(f"generate_captions(): pass a list of strings, got the string {strings!r}")
                kwargs[name] = [list(processor.tokenizer(s, add_special_tokens=False)["input_ids"]) for s in strings]
        if device is None:
            device = self.device
        if images is not None:
            assert pixel_values is None, "you can only pass either images or visual features to generate_captions()!"
            if not isinstance(images, (list, tuple)):
                images = [images]
            pixel_values = processor(images=images, device=device)["pixel_values"]
        assert pixel_values is not None, "you must pass either images or visual features to generate_captions()!"
        batch_size = pixel_values.size(0)
        input_ids, media_locations, attention_mask = processor.encode_text(prompt, device)
        input_ids = input_ids[:1].expand(batch_size, -1).contiguous()
        media_locations = media_locations[:1].expand(batch_size, -1).contiguous()
        attention_mask = attention_mask[:1].expand(batch_size, -1).contiguous()
        lm_cfg = self.flamingo.lm.config
        if pixel_values.ndim == 4:
            pixel_values = pixel_values[:, None]       # (b c h w) -> one image per sequence
        if return_scores:                              # the scores come with the output object; sampling and greedy need the token values for them
            kwargs = dict(kwargs, return_dict_in_generate=True, output_logprobs=num_beams <= 1)
        out = self.generate(inputs=input_ids, media_locations=media_locations, attention_mask=attention_mask, pixel_values=pixel_values,
                            num_beams=num_beams, early_stopping=True, use_cache=True, bos_token_id=lm_cfg.bos_token_id,
                            eos_token_id=lm_cfg.eos_token_id, pad_token_id=lm_cfg.eos_token_id, max_length=max_length, **kwargs)
        out_ids = out.sequences if isinstance(out, D.GenerateOutput) else out
        captions = [processor.remove_tags(t) for t in processor.tokenizer.batch_decode(out_ids, skip_special_tokens=True)]
        n = kwargs.get("num_return_sequences", 1)
        group = (lambda v: [v[i:i + n] for i in range(0, len(v), n)]) if n > 1 else (lambda v: v)
        if return_scores:
            return group(captions), group([float(s) for s in out.sequences_scores.tolist()])
        return group(captions)

    @torch.no_grad()
    def score_candidates(self, input_ids, media_locations, attention_mask=None, pixel_values=None, visual_features=None, *,
                         candidate_ids, eos_token_id: Optional[int] = None, max_rows: int = 1024) -> D.CandidateScores:
        """EXACT closed-set scoring (classification, multiple choice, yes / no, reranking): for every sequence s of the batch and every
        candidate j of ONE candidate set (lists of token ids, as generate(candidate_ids=)),
            logprobs[s, j] = sum_t log p(c_j[t] | media_s, prompt_s, c_j[:t])   (+ log p(eos | media_s, prompt_s, c_j) with eos_token_id)
        in a decoding.CandidateScores (logprobs (b, k) float32 - float64 for a float64 model -, token_counts (k,)).  Columns follow the
        caller's order; duplicate candidates get equal columns; a candidate that is a prefix of another is fine, and with eos scored the
        two become comparable.  Unlike generate(candidate_ids=) this is no search and nothing is renormalised over the allowed tokens:
        calibration, top-k accuracy and ranking metrics can be computed from it.
        The visuals are encoded once, the prompt runs once per sequence and group through the cross-attention / LM caches, and every
        distinct candidate prefix runs once: decoding.score_trie walks the candidates' trie level by level, one LM step and one launch of
        ff_logprob_gather per level (functional.logprob_gather reads the queried tokens' log-probabilities from the step's logits in the
        model's dtype - no float32 copy, no vocabulary-wide log-softmax); on CPU tensors the same walk runs with
        decoding.logprob_gather_torch.  `max_rows` bounds the LM batch of a level: the first tokens' subtrees are split into groups whose
        widest level times b stays within it (one subtree wider than that runs alone); every group re-runs the b-row prompt step, the
        visuals are never encoded twice.  The path is dynamic - shapes change per level, no graph is captured, no decode session is built.
        ValueError: no candidates, an empty one, an id outside the vocabulary, a candidate that contains eos; max_rows not an int >= 1."""
        am = attention_mask if attention_mask is not None else torch.ones_like(input_ids)
        if visual_features is None and pixel_values is not None:         # encoded once, whatever the number of groups
            visual_features, pixel_values = self.flamingo.encode_resample_visuals(pixel_values), None
        return D.score_trie(self._score_step, self._reorder_cache, input_ids, media_locations, am, pixel_values, visual_features,
                            candidate_ids, self.flamingo.lm.config.vocab_size, eos=eos_token_id, max_rows=max_rows)

    @torch.no_grad()
    def classify(self, processor, pixel_values=None, images=None, prompt: str = "<image>", candidates=None, score_eos: bool = False,
                 normalize: Optional[str] = None, max_rows: int = 1024):
        """Closed-set classification of a batch of images over strings: (labels, probs), `labels` the best candidate string per image,
        `probs` (b, k) the softmax over the candidates of the ranked quantity - score_candidates' logprobs with normalize=None, logprobs /
        token_counts with normalize="tokens" (anything else: ValueError).  The prompt is replicated for every image; every candidate is
        tokenised VERBATIM with processor.tokenizer(s, add_special_tokens=False), as generate_captions(candidates=) does (a leading space
        is the caller's business).  score_eos=True also scores the LM's eos after each candidate, which makes a candidate comparable
        with its own extensions."""
        if normalize not in (None, "tokens"):
            raise ValueError(f"classify(): normalize must be None or 'tokens', got {normalize!r}")
        if candidates is None or isinstance(candidates, str):
            raise ValueError(f"classify(): pass a list of strings, got {'the string ' if isinstance(candidates, str) else ''}{candidates!r}")
        candidates = list(candidates)
        cand_ids = [list(processor.tokenizer(s, add_special_tokens=False)["input_ids"]) for s in candidates]
        device = self.device
        if images is not None:
            assert pixel_values is None, "you can only pass either images or visual features to classify()!"
            if not isinstance(images, (list, tuple)):
                images = [images]
            pixel_values = processor(images=images, device=device)["pixel_values"]
        assert pixel_values is not None, "you must pass either images or visual features to classify()!"
        batch_size = pixel_values.size(0)
        input_ids, media_locations, attention_mask = processor.encode_text(prompt, device)
        input_ids = input_ids[:1].expand(batch_size, -1).contiguous()
        media_locations = media_locations[:1].expand(batch_size, -1).contiguous()
        attention_mask = attention_mask[:1].expand(batch_size, -1).contiguous()
        if pixel_values.ndim == 4:
            pixel_values = pixel_values[:, None]       # (b c h w) -> one image per sequence
        res = self.score_candidates(input_ids, media_locations, attention_mask, pixel_values=pixel_values, candidate_ids=cand_ids,
                                    eos_token_id=self.flamingo.lm.config.eos_token_id if score_eos else None, max_rows=max_rows)
        ranked = res.logprobs if normalize is None else res.logprobs / res.token_counts.to(res.logprobs.dtype)
        probs = ranked.softmax(-1)
        return [candidates[i] for i in probs.argmax(-1).tolist()], probs

    @torch.no_grad()
    def score_sequences(self, input_ids, media_locations, attention_mask, pixel_values=None, visual_features=None,
                        k: int = 100000) -> torch.Tensor:
        """Zero-shot scoring as the reference has it (:607-712): the log-prob of each candidate sequence given the same visuals.  Kept for
        parity.  For EXACT scores of a closed set - every candidate's log-probability for a whole batch, shared prefixes run once, no
        vocabulary-wide log-softmax - use score_candidates() (or classify() on strings); for SEARCH use constrained decoding,
        generate(..., candidate_ids=, return_dict_in_generate=True, output_logprobs=True) - greedy or beam search restricted to the trie of
        the candidates inside the cached, graph-replayed decode step, sequences_scores / token_logprobs giving the chosen candidate's
        probability over the allowed set and num_return_sequences a top-n - which runs the prefix once and never materialises a per-candidate
        log-softmax.  This method recomputes the LM prefix for every candidate and holds a (k, L, vocab) float32 log-softmax (1 GB for 1000
        class names of 5 tokens at vocab 50258).  The shared prefix is run once with use_cache; its cross-attention K/V are reused for the
        candidates (the LM self-attention prefix is recomputed: HF Cache objects are not sliceable per candidate)."""
        assert visual_features is None or visual_features.ndim == 3
        n_choices = input_ids.size(0)
        n_reuse = get_common_prefix_length(input_ids)
        k = min(k, n_choices)
        out = self.flamingo(input_ids=input_ids[:1, :n_reuse], media_locations=media_locations[:1, :n_reuse],
                            attention_mask=attention_mask[:1, :n_reuse],
                            pixel_values=pixel_values.unsqueeze(0) if pixel_values is not None else None,
                            visual_features=visual_features.unsqueeze(0) if visual_features is not None else None, use_cache=True)
        next_tokens = input_ids[:, n_reuse]
        topk = out.logits[0, -1, :].index_select(0, next_tokens).topk(k).indices
        xattn_past = [tuple(t.expand(k, *t.shape[1:]) for t in kv) for kv in out.past_key_values[0]]
        out2 = self.flamingo(input_ids=input_ids[topk], media_locations=media_locations[topk], attention_mask=attention_mask[topk],
                             past_key_values=(xattn_past, None))
        logp = out2.logits[:, n_reuse - 1:-1].float().log_softmax(-1)
        tgt = input_ids[topk][:, n_reuse:]
        tok = logp.gather(-1, tgt[..., None])[..., 0]     # every position after the shared prefix counts, padded or not (reference :699-703: unmasked sum)
        scores = torch.full([n_choices], torch.finfo(torch.float).min, device=tok.device)
        scores[topk] = tok.sum(1)
        return scores.detach()
