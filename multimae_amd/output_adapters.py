"""Output adapters (mirror of the reference's ``multimae/output_adapters.py`` for the
pre-training path).

Reference: SpatialOutputAdapter output_adapters.py:33-282.  Same constructor, same parameter
names and registration order (mask_token, pos_emb, task_embeddings, decoder.{q,kv,proj},
{context,query,out}_norm, mlp, decoder_transformer.*, out_proj, proj_context registered last
in init()).  forward() is ONE autograd node (functions.SpatialAdapterFn) whose forward and
backward are fixed HIP kernel sequences; the (B, N_total, D) mask-token tensor of the
reference is never materialised.

LinearOutputAdapter (output_adapters.py:285-356, the classification head of the MultiViT fine-tuning forward,
SURVEY.md section 8f row 4) is built on the same kernels.  ConvNeXtAdapter (output_adapters.py:481-573, the default head of
run_finetuning_semseg.py) is one autograd node (functions.ConvNeXtHeadFn) on the row kernels, the GEMMs and csrc/convnext.hip.
DPTOutputAdapter (output_adapters.py:576-759, the head of every shipped depth and Taskonomy recipe) is built with the regression head
type: ten autograd nodes (functions.DPTReassembleFn x 4, the fusion blocks of output_adapter_utils.py, functions.DPTHeadFn) on
csrc/dpt.hip, csrc/conv3x3.hip and the GEMMs.  SegmenterMaskTransformerAdapter is not built: its name exists so that the semseg
script's import line works, and constructing it raises NotImplementedError.
"""
from __future__ import annotations

from functools import partial
from typing import Dict, Iterable, List, Optional, Tuple, Union

import torch
import torch.nn.functional as F
from torch import nn

from . import engine
from .functions import ConvNeXtHeadFn, DPTHeadFn, DPTReassembleFn, ImageMark, SpatialAdapterFn, TokenMeanFn
from .output_adapter_utils import Conv3x3, Interpolate, _conv_cfg, make_fusion_block, make_scratch
from .multimae_utils import (Block, CrossAttention, LayerNorm, Linear, Mlp, _as_hip_norm, _cfg, bias_or_zero, block_params,
                             build_2d_sincos_posemb, pair, trunc_normal_)


class SpatialOutputAdapter(nn.Module):
    """Cross-attention decoder for spatial outputs (output_adapters.py:33-142)."""

    def __init__(self, num_channels: int, stride_level: int, patch_size_full: Union[int, Tuple[int, int]],
                 dim_tokens_enc: Optional[int] = None, dim_tokens: int = 256, depth: int = 0, learnable_pos_emb: int = False,
                 image_size: Union[int, Tuple[int]] = 224, mlp_ratio: int = 4.0, num_heads: int = 8, qkv_bias: bool = True,
                 drop_rate: float = 0.0, attn_drop_rate: float = 0.0, drop_path_rate: float = 0.0,
                 norm_layer: nn.Module = partial(nn.LayerNorm, eps=1e-6), use_task_queries: bool = True,
                 task: Optional[str] = None, context_tasks: Optional[list] = None, use_xattn: bool = True):
        super().__init__()
        self.num_channels = num_channels
        self.stride_level = stride_level
        self.patch_size_full = pair(patch_size_full)
        self.dim_tokens_enc = dim_tokens_enc
        self.dim_tokens = dim_tokens
        self.learnable_pos_emb = learnable_pos_emb
        self.image_size = pair(image_size)
        self.use_task_queries = use_task_queries
        self.task = task
        self.use_xattn = use_xattn
        self.num_heads = num_heads
        self.depth = depth
        self._drop_rates = (float(attn_drop_rate), float(drop_rate))
        if learnable_pos_emb:
            # (the reference allocates this table as (1, h, w, D) but resizes it with F.interpolate as if it were (1, D, h, w),
            # output_adapters.py:108-111,172: not a behaviour worth mirroring)
            raise NotImplementedError('learnable decoder positional embeddings are not built in the HIP engine')
        # (drop_rate / attn_drop_rate > 0: the nn.Dropout sites of the cross attention and of the decoder blocks run as element-wise
        # passes between the per-kernel sequence of the adapter; 0 -- every shipped configuration -- keeps the one-call adapter)
        # (drop_path_rate > 0: stochastic depth in decoder_transformer, output_adapters.py:126-132 -- the per-sample scales are drawn in
        # forward() in the reference's order and folded into the blocks' residual adds, as in the encoder)

        self.P_H = max(1, self.patch_size_full[0] // stride_level)
        self.P_W = max(1, self.patch_size_full[1] // stride_level)

        if context_tasks is not None:
            self.task_embeddings = nn.ParameterDict(
                {t: nn.Parameter(torch.zeros(1, 1, self.dim_tokens)) for t in context_tasks})
            for embedding in self.task_embeddings.values():
                trunc_normal_(embedding, std=0.02)
        else:
            self.task_embeddings = None

        self.mask_token = nn.Parameter(torch.zeros(1, 1, self.dim_tokens))

        h_posemb = self.image_size[0] // (self.stride_level * self.P_H)
        w_posemb = self.image_size[1] // (self.stride_level * self.P_W)
        self.pos_emb = nn.Parameter(build_2d_sincos_posemb(h=h_posemb, w=w_posemb, embed_dim=self.dim_tokens),
                                    requires_grad=False)

        self._eps = _as_hip_norm(norm_layer, self.dim_tokens).eps
        if self.use_xattn:           # output_adapters.py:114-123: without it the queries go straight into decoder_transformer
            self.decoder = CrossAttention(dim=self.dim_tokens, num_heads=num_heads, qkv_bias=qkv_bias,
                                          attn_drop=attn_drop_rate, proj_drop=drop_rate)
            self.context_norm = _as_hip_norm(norm_layer, self.dim_tokens)
            self.query_norm = _as_hip_norm(norm_layer, self.dim_tokens)
            self.out_norm = _as_hip_norm(norm_layer, self.dim_tokens)
            mlp_hidden_dim = int(self.dim_tokens * mlp_ratio)
            self.mlp = Mlp(in_features=self.dim_tokens, hidden_features=mlp_hidden_dim)

        if depth > 0:
            dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
            self.decoder_transformer = nn.Sequential(*[
                Block(dim=self.dim_tokens, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop=drop_rate,
                      attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer) for i in range(depth)])
        else:
            self.decoder_transformer = nn.Identity()

        self.dim_patch = self.num_channels * self.P_H * self.P_W
        self.out_proj = Linear(self.dim_tokens, self.dim_patch)

        if self.dim_tokens_enc is not None:
            self.init(dim_tokens_enc=dim_tokens_enc)

    def init(self, dim_tokens_enc: int = 768):
        self.dim_tokens_enc = dim_tokens_enc
        self.proj_context = Linear(self.dim_tokens_enc, self.dim_tokens)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'pos_emb', 'mask_token', 'task_embeddings'}

    def _pos_tokens(self, nh: int, nw: int) -> torch.Tensor:
        """bilinear-resized decoder pos-emb as (nh*nw, D) (output_adapters.py:172-173), cached."""
        p = self.pos_emb
        key = (nh, nw, p._version, p.device, p.data_ptr())
        cache = self.__dict__.setdefault('_pos_cache', {})
        t = cache.get(key)
        if t is None:
            cache.clear()
            with torch.no_grad():
                r = F.interpolate(p.detach(), size=(nh, nw), mode='bilinear', align_corners=False)
                t = r[0].flatten(1).t().contiguous().float()
            cache[key] = t
        return t

    def _params(self, in_tasks):
        te = []
        for t in in_tasks:
            if self.task_embeddings is not None and t in self.task_embeddings:
                te.append(self.task_embeddings[t])
            else:
                te.append(None)
        if not self.use_xattn:
            ps = [self.mask_token, *te] + [None] * 16
            if self.depth > 0:
                for blk in self.decoder_transformer:
                    ps += block_params(blk)
            return ps + [self.out_proj.weight, self.out_proj.bias, self.proj_context.weight, self.proj_context.bias]
        d = self.decoder
        ps = [self.mask_token, *te, d.q.weight, bias_or_zero(d.q, getattr(d, '_zero_q_bias', None)), d.kv.weight,
              bias_or_zero(d.kv, getattr(d, '_zero_kv_bias', None)), d.proj.weight, d.proj.bias,
              self.context_norm.weight, self.context_norm.bias, self.query_norm.weight, self.query_norm.bias,
              self.out_norm.weight, self.out_norm.bias, self.mlp.fc1.weight, self.mlp.fc1.bias, self.mlp.fc2.weight,
              self.mlp.fc2.bias]
        if self.depth > 0:
            for blk in self.decoder_transformer:
                ps += block_params(blk)
        ps += [self.out_proj.weight, self.out_proj.bias, self.proj_context.weight, self.proj_context.bias]
        return ps

    def forward(self, encoder_tokens: torch.Tensor, input_info: Dict, ids_keep: torch.Tensor, ids_restore: torch.Tensor,
                act_dtype: Optional[torch.dtype] = None, on_done=None, f32_gemm: str = 'exact',
                encoder_tokens_act: Optional[torch.Tensor] = None):
        """(B, n_keep+G, D_enc) encoder tokens -> (B, C, H_t, W_t) prediction (output_adapters.py:236-282)."""
        assert self.dim_tokens_enc is not None, 'Need to call init(dim_tokens_enc) function first'
        if self.task_embeddings is None:
            raise AttributeError('SpatialOutputAdapter built with context_tasks=None has no task_embeddings '
                                 '(the reference raises here too, output_adapters.py:166)')
        H, W = input_info['image_size']
        nh = H // (self.stride_level * self.P_H)
        nw = W // (self.stride_level * self.P_W)
        in_tasks = list(input_info['tasks'].keys())
        # queries (output_adapters.py:208-220): the task's own rows of the unshuffled context, or -- when the task is not an
        # encoder input (e.g. --in_domains rgb --out_domains rgb-depth-semseg) or use_task_queries=False -- mask_token + pos
        # (+ the task's embedding if the adapter has one) on every grid position
        task_queries = bool(self.use_task_queries and self.task in input_info['tasks'])
        offs = [0]
        for t in in_tasks:
            n = input_info['tasks'][t]['num_tokens']
            assert n == nh * nw, 'all tasks must share the decoder token grid (output_adapters.py:175)'
            offs.append(offs[-1] + n)
        G = input_info.get('num_global_tokens', 0)
        cfg = _cfg(self, act=act_dtype, heads=self.num_heads, eps=self._eps, use_xattn=self.use_xattn, task_offsets=offs,
                   q_task=in_tasks.index(self.task) if task_queries else -1, G=G, D=self.dim_tokens, pos=self._pos_tokens(nh, nw), depth=self.depth,
                   C=self.num_channels, nh=nh, nw=nw, ph=self.P_H, pw=self.P_W, on_done=on_done, f32_gemm=f32_gemm,
                   enc_act=encoder_tokens_act)
        if self.depth > 0:                                   # two draws per block with a rate > 0, block by block, all up front (see _stack_drop_path on the stream order)
            from .multimae_utils import _stack_drop_path
            cfg.dp = _stack_drop_path(list(self.decoder_transformer), encoder_tokens.shape[0], encoder_tokens.device)
        if self.training and any(r > 0. for r in self._drop_rates):
            cfg.drops = self._drop_rates
        params = self._params(in_tasks)
        if not task_queries and self.task_embeddings is not None and self.task in self.task_embeddings:
            # the query rows are mask_token + task_embeddings[task] + pos: one vector added to every row, passed in the mask-token
            # slot (the kernels use that slot for nothing else in this mode); autograd splits its gradient between the two
            params[0] = self.mask_token + self.task_embeddings[self.task]
        img, token = SpatialAdapterFn.apply(cfg, encoder_tokens, ids_keep.contiguous(), ids_restore.contiguous(), *params)
        if getattr(cfg, 'lazy_fill', None) is not None or cfg.handle is not None:
            # written when first read (the masked losses never read it); already written when the adapter ran eagerly -- the wrapper
            # then only carries the patch-row side channel through clone() (torch DDP's output sink)
            from .lazy import LazyPrediction
            img = LazyPrediction.wrap(img, getattr(cfg, 'lazy_fill', None))
            cfg.lazy_fill = None
        if cfg.handle is not None:
            img._mmae_pat = cfg.handle       # a masked loss applied to exactly this tensor works on the patch rows (criterion.py)
        return img


class LinearOutputAdapter(nn.Module):
    """Linear classification head (output_adapters.py:285-356): mean over the encoder tokens (or the last = global token),
    LayerNorm, Linear.  Same constructor, parameter names (norm.*, head.*) and seeded initialisation as the reference."""

    def __init__(self, num_classes: int, dim_tokens_enc: Optional[int] = None, use_mean_pooling: bool = True,
                 norm_layer: nn.Module = partial(nn.LayerNorm, eps=1e-6), init_scale: float = 1.0):
        super().__init__()
        self.num_classes = num_classes
        self.dim_tokens_enc = dim_tokens_enc
        self.use_mean_pooling = use_mean_pooling
        self.norm_layer = norm_layer
        self.init_scale = init_scale
        if self.dim_tokens_enc is not None:
            self.init(dim_tokens_enc=dim_tokens_enc)

    def init(self, dim_tokens_enc: int = 768):
        self.dim_tokens_enc = dim_tokens_enc
        self.norm = _as_hip_norm(self.norm_layer, self.dim_tokens_enc)
        self.head = Linear(dim_tokens_enc, self.num_classes) if self.num_classes > 0 else nn.Identity()
        self.apply(self._init_weights)
        if self.num_classes > 0:
            self.head.weight.data.mul_(self.init_scale)
            self.head.bias.data.mul_(self.init_scale)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def get_classifier(self):
        return self.head

    def reset_classifier(self, num_classes, global_pool=''):
        self.num_classes = num_classes
        self.init(dim_tokens_enc=self.dim_tokens_enc)

    def forward(self, encoder_tokens: torch.Tensor, **kwargs):
        if self.use_mean_pooling:
            x = TokenMeanFn.apply(encoder_tokens)
        else:
            x = encoder_tokens[:, -1]                       # the global token is appended last (multimae.py:344-347)
        return self.head(self.norm(x))


class ConvNeXtBlock(nn.Module):
    """Parameter container of the reference's ConvNeXtBlock(dim) (output_adapter_utils.py:19-57) as ConvNeXtAdapter builds it: no layer
    scale, no drop path.  Same modules in the same order, so construction draws the same random numbers.  The computation is
    ConvNeXtHeadFn's (the head runs as one node)."""

    def __init__(self, dim: int):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = Linear(dim, 4 * dim)
        self.pwconv2 = Linear(4 * dim, dim)


class ConvNeXtAdapter(nn.Module):
    """ConvNeXt semantic-segmentation head (output_adapters.py:481-573): the main tasks' token rows concatenated along features,
    proj_dec, a pixel shuffle into a map of C = embed_dim / preds_per_patch channels at sqrt(preds_per_patch) times the token grid,
    `depth` ConvNeXt blocks, a 1 x 1 final_layer and F.interpolate to the image size.  Same constructor, parameter names,
    registration order and seeded initialisation as the reference (proj_dec registered last, in init())."""

    def __init__(self, num_classes, embed_dim: int = 6144, preds_per_patch: int = 16, main_tasks: Iterable[str] = ('rgb',),
                 patch_size: int = 16, depth: int = 4, interpolate_mode: str = 'bilinear', **kwargs):
        super().__init__()
        s = int(round(preds_per_patch ** 0.5))
        if preds_per_patch < 1 or s * s != preds_per_patch:
            raise ValueError(f'ConvNeXtAdapter: preds_per_patch = {preds_per_patch} is not a perfect square')
        if embed_dim % preds_per_patch != 0:
            raise ValueError(f'ConvNeXtAdapter: embed_dim = {embed_dim} is not a multiple of preds_per_patch = {preds_per_patch}')
        if interpolate_mode not in ('bilinear', 'nearest'):
            raise NotImplementedError(f'ConvNeXtAdapter: interpolate_mode {interpolate_mode!r} is not built (bilinear, nearest)')
        self.main_tasks = main_tasks
        self.patch_size = patch_size
        self.embed_dim = embed_dim
        self.preds_per_patch = preds_per_patch
        self.class_dim = embed_dim // preds_per_patch
        self.num_classes = num_classes
        self.interpolate_mode = interpolate_mode
        self.blocks = nn.Sequential(*[ConvNeXtBlock(dim=self.class_dim) for _ in range(depth)])
        self.final_layer = nn.Conv2d(self.class_dim, self.num_classes, 1)
        self.apply(self._init_weights)

    def init(self, dim_tokens_enc: int = 768):
        self.in_channels = dim_tokens_enc * len(self.main_tasks)
        self.proj_dec = Linear(self.in_channels, self.embed_dim)
        self._init_weights(self.proj_dec)

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def _params(self):
        ps = []
        for b in self.blocks:
            ps += [b.dwconv.weight, b.dwconv.bias, b.norm.weight, b.norm.bias, b.pwconv1.weight, b.pwconv1.bias, b.pwconv2.weight,
                   b.pwconv2.bias]
        return ps + [self.final_layer.weight, self.final_layer.bias, self.proj_dec.weight, self.proj_dec.bias]

    def forward(self, encoder_tokens: torch.Tensor, input_info: Dict):
        """(B, N_total, D) encoder tokens -> f32 (B, num_classes, H, W) logits (output_adapters.py:552-570)."""
        H, W = input_info['image_size']
        NH, NW = H // self.patch_size, W // self.patch_size
        starts, counts = [], []
        for task in self.main_tasks:
            info = input_info['tasks'][task]
            starts.append(int(info['start_idx']))
            counts.append(int(info['end_idx']) - int(info['start_idx']))
        if len(set(counts)) != 1 or counts[0] != NH * NW:
            raise ValueError(f'ConvNeXtAdapter: the main tasks {tuple(self.main_tasks)} have {counts} tokens; each needs the '
                             f'{NH} x {NW} grid of the {H} x {W} image')
        D = encoder_tokens.shape[-1]
        if D * len(starts) != self.in_channels:
            raise ValueError(f'ConvNeXtAdapter: encoder width {D} x {len(starts)} tasks != proj_dec input {self.in_channels}')
        C = self.class_dim
        cfg = _cfg(self, starts=starts, N=NH * NW, NH=NH, NW=NW, s=int(round(self.preds_per_patch ** 0.5)), C=C, K=self.num_classes,
                   H=H, W=W, depth=len(self.blocks), mode=self.interpolate_mode, eps=1e-6)
        if C % 4 or C > 1024:
            raise ValueError(f'ConvNeXtAdapter: the LayerNorm kernel needs embed_dim / preds_per_patch ({C}) to be a multiple of 4 '
                             'in [4, 1024]')
        if cfg.act != torch.float32 and (C % 8 or self.in_channels % 8):
            raise ValueError(f'ConvNeXtAdapter: the bf16 GEMMs need embed_dim / preds_per_patch ({C}) and the concatenated token width '
                             f'({self.in_channels}) to be multiples of 8; use engine.set_precision("fp32") for this geometry')
        img, _ = ConvNeXtHeadFn.apply(cfg, encoder_tokens, *self._params())
        if getattr(cfg, 'lazy_fill', None) is not None or cfg.handle is not None:
            # written when first read (criterion.SegCrossEntropyLoss and metrics.seg_argmax work on the low-resolution logits and never
            # read it); already written when the head ran eagerly -- the wrapper then only carries the side channel through clone()
            from .lazy import LazyPrediction
            img = LazyPrediction.wrap(img, getattr(cfg, 'lazy_fill', None))
            cfg.lazy_fill = None
        if cfg.handle is not None:
            img._mmae_seg = cfg.handle       # functions.SegHandle: the logits behind exactly this tensor
        return img


class DPTOutputAdapter(nn.Module):
    """DPT head (output_adapters.py:576-759) with the regression head type, the one every shipped depth and Taskonomy recipe uses:
    four hooked encoder layers are reassembled into maps at 4x, 2x, 1x and 1/2x the token grid (act_1..4_postprocess), projected to
    feature_dim (scratch.layer_rn), fused coarse to fine by four RefineNet blocks (scratch.refinenet4..1) and turned into a
    (B, num_classes, H, W) f32 image by the head.  Same constructor signature, attribute names, parameter names, registration order
    and seeded initialisation as the reference: at the reference's default geometry the state_dict has its 82 keys in its order, and
    a reference DPT checkpoint loads with load_state_dict(strict=True).  nn.ConvTranspose2d / nn.Conv2d are parameter holders.

    forward() takes the list of all encoder layers' tokens (MultiViT.forward(return_all_layers=True)) and runs ten autograd nodes:
    four functions.DPTReassembleFn, the four fusion blocks, functions.DPTHeadFn.  The prediction is a plain contiguous NCHW tensor
    (no LazyPrediction, no low-resolution handle: the head's output is at image resolution already).  With
    engine.patch_domain_loss() on and no capture running it carries ``_mmae_img`` (functions.ImageMark), by which the regression
    losses and the depth metrics recognise it and run their fused kernels on the image.

    Not built (NotImplementedError naming the argument): use_bn=True, head_type='semseg', num_classes > 16 (the regression tail
    kernel keeps one accumulator per output channel in registers; 16 is also the limit of the regression losses on the ConvNeXt head's map).  The token grid
    must be even in both directions (the reference fails on an odd one as well).  bf16 mode needs every channel count to be a
    multiple of 8 (ValueError); engine.set_precision('fp32') runs every product on the exact-f32 path and takes any.  The head runs
    uncaptured only: it is untested under graph capture, as the fusion blocks."""

    MAX_CLASSES = 16             # == ops.DPT_TAIL_MAX_K

    def __init__(self, num_classes: int = 3, stride_level: int = 1, patch_size: Union[int, Tuple[int, int]] = 16,
                 main_tasks: Iterable[str] = ('rgb',), hooks: List[int] = [2, 5, 8, 11], layer_dims: List[int] = [96, 192, 384, 768],
                 feature_dim: int = 256, use_bn: bool = False, dim_tokens_enc: Optional[int] = None, head_type: str = 'regression',
                 **kwargs):
        super().__init__()
        if head_type not in ('regression', 'semseg'):
            raise ValueError(f'DPTOutputAdapter: head_type must be "regression" or "semseg", got {head_type!r}')
        if head_type == 'semseg':
            raise NotImplementedError("DPTOutputAdapter: head_type = 'semseg' is not built in multimae_amd (its Dropout and optional "
                                      "BatchNorm are further work); the regression head is")
        if use_bn:
            raise NotImplementedError('DPTOutputAdapter: use_bn = True is not built in multimae_amd')
        if num_classes > self.MAX_CLASSES:
            raise NotImplementedError(f'DPTOutputAdapter: num_classes = {num_classes} > {self.MAX_CLASSES} is not built in multimae_amd '
                                      '(the regression tail kernel keeps one accumulator per output channel in registers)')
        if num_classes < 1:
            raise ValueError(f'DPTOutputAdapter: num_classes = {num_classes} must be at least 1')
        self.num_channels = num_classes
        self.stride_level = stride_level
        self.patch_size = pair(patch_size)
        self.main_tasks = main_tasks
        self.hooks = hooks
        self.layer_dims = layer_dims
        self.feature_dim = feature_dim
        self.dim_tokens_enc = dim_tokens_enc * len(self.main_tasks) if dim_tokens_enc is not None else None
        self.head_type = head_type

        self.P_H = max(1, self.patch_size[0] // stride_level)
        self.P_W = max(1, self.patch_size[1] // stride_level)

        self.scratch = make_scratch(layer_dims, feature_dim, groups=1, expand=False)
        self.scratch.refinenet1 = make_fusion_block(feature_dim, use_bn)
        self.scratch.refinenet2 = make_fusion_block(feature_dim, use_bn)
        self.scratch.refinenet3 = make_fusion_block(feature_dim, use_bn)
        self.scratch.refinenet4 = make_fusion_block(feature_dim, use_bn)

        # the "DPTDepthModel" head (output_adapters.py:627-633); run as one node by forward(), the modules hold the parameters
        self.head = nn.Sequential(
            Conv3x3(feature_dim, feature_dim // 2, stride=1, bias=True),
            Interpolate(scale_factor=2, mode='bilinear', align_corners=True),
            Conv3x3(feature_dim // 2, 32, stride=1, bias=True),
            nn.ReLU(True),
            nn.Conv2d(32, self.num_channels, kernel_size=1, stride=1, padding=0))

        if self.dim_tokens_enc is not None:
            self.init(dim_tokens_enc=dim_tokens_enc)

    def init(self, dim_tokens_enc: int = 768):
        """the parts that depend on the encoder width (output_adapters.py:650-715): act_1..4_postprocess, also listed in
        act_postprocess (both sets of keys appear in a state_dict, as in the reference)"""
        self.dim_tokens_enc = dim_tokens_enc * len(self.main_tasks)
        D, L = self.dim_tokens_enc, self.layer_dims
        self.act_1_postprocess = nn.Sequential(
            nn.Conv2d(in_channels=D, out_channels=L[0], kernel_size=1, stride=1, padding=0),
            nn.ConvTranspose2d(in_channels=L[0], out_channels=L[0], kernel_size=4, stride=4, padding=0, bias=True, dilation=1, groups=1))
        self.act_2_postprocess = nn.Sequential(
            nn.Conv2d(in_channels=D, out_channels=L[1], kernel_size=1, stride=1, padding=0),
            nn.ConvTranspose2d(in_channels=L[1], out_channels=L[1], kernel_size=2, stride=2, padding=0, bias=True, dilation=1, groups=1))
        self.act_3_postprocess = nn.Sequential(
            nn.Conv2d(in_channels=D, out_channels=L[2], kernel_size=1, stride=1, padding=0))
        self.act_4_postprocess = nn.Sequential(
            nn.Conv2d(in_channels=D, out_channels=L[3], kernel_size=1, stride=1, padding=0),
            nn.Conv2d(in_channels=L[3], out_channels=L[3], kernel_size=3, stride=2, padding=1))
        self.act_postprocess = nn.ModuleList([self.act_1_postprocess, self.act_2_postprocess, self.act_3_postprocess,
                                              self.act_4_postprocess])

    def _layer_params(self, i: int):
        ps = []
        for m in self.act_postprocess[i]:
            ps += [m.weight, m.bias]
        return ps + [self.scratch.layer_rn[i].weight]

    def forward(self, encoder_tokens: List[torch.Tensor], input_info: Dict):
        """list of (B, N_total, D) encoder-layer tokens -> f32 (B, num_classes, H, W) prediction (output_adapters.py:728-759)"""
        if self.dim_tokens_enc is None or not hasattr(self, 'act_postprocess'):
            raise ValueError('DPTOutputAdapter: init(dim_tokens_enc) must be called before forward()')
        if isinstance(encoder_tokens, torch.Tensor) or len(encoder_tokens) < max(self.hooks) + 1:
            n = 1 if isinstance(encoder_tokens, torch.Tensor) else len(encoder_tokens)
            raise ValueError(f'DPTOutputAdapter: encoder_tokens must list the tokens of every encoder layer up to hook {max(self.hooks)} '
                             f'(MultiViT.forward(return_all_layers=True)); got {n}')
        H, W = input_info['image_size']
        NH = H // (self.stride_level * self.P_H)
        NW = W // (self.stride_level * self.P_W)
        starts, counts = [], []
        for task in self.main_tasks:
            info = input_info['tasks'][task]
            starts.append(int(info['start_idx']))
            counts.append(int(info['end_idx']) - int(info['start_idx']))
        if len(set(counts)) != 1 or counts[0] != NH * NW:
            raise ValueError(f'DPTOutputAdapter: the main_tasks {tuple(self.main_tasks)} have {counts} tokens; each needs the '
                             f'{NH} x {NW} grid of the {H} x {W} image')
        layers = [encoder_tokens[hook] for hook in self.hooks]
        D = layers[0].shape[-1]
        if any(l.dim() != 3 or l.shape != layers[0].shape for l in layers) or D * len(starts) != self.dim_tokens_enc:
            raise ValueError(f'DPTOutputAdapter: encoder width {D} x {len(starts)} tasks != the dim_tokens_enc of init() '
                             f'({self.dim_tokens_enc}), or the hooked layers differ in shape')
        if NH % 2 or NW % 2:
            raise ValueError(f'DPTOutputAdapter: the token grid N_H x N_W = {NH} x {NW} must be even in both directions (act_4_postprocess '
                             'halves it and refinenet4 doubles it again; the reference fails on an odd grid too)')
        cfg0 = _conv_cfg(self)
        chans = (self.dim_tokens_enc, *self.layer_dims, self.feature_dim, self.feature_dim // 2)
        if cfg0.act != torch.float32 and any(c % 8 for c in chans):
            raise ValueError(f'DPTOutputAdapter: the bf16 gathers and GEMMs need channel counts that are multiples of 8 (dim_tokens_enc x '
                             f'tasks, layer_dims, feature_dim, feature_dim // 2 = {chans}); use engine.set_precision("fp32") for this geometry')
        maps = []
        for i, tok in enumerate(layers):
            cfg = _conv_cfg(self, layer=i, starts=starts, N=NH * NW, NH=NH, NW=NW)
            maps.append(DPTReassembleFn.apply(cfg, tok, *self._layer_params(i)))
        path_4 = self.scratch.refinenet4(maps[3])
        path_3 = self.scratch.refinenet3(path_4, maps[2])
        path_2 = self.scratch.refinenet2(path_3, maps[1])
        path_1 = self.scratch.refinenet1(path_2, maps[0])
        h = self.head
        out = DPTHeadFn.apply(cfg0, path_1, h[0].weight, h[0].bias, h[2].weight, h[2].bias, h[4].weight, h[4].bias)
        if engine.patch_domain_loss() and engine.capturing() is None and not (out.is_cuda and torch.cuda.is_current_stream_capturing()):
            # the regression losses and the depth metrics run their fused kernels on exactly this tensor while it is unmodified
            # (criterion._image_fused_ok); still a plain torch.Tensor, and no low-resolution handle
            out._mmae_img = ImageMark(out.shape, out._version)
        return out


class SegmenterMaskTransformerAdapter(nn.Module):
    """Name only (output_adapters.py:359-478): the Segmenter mask-transformer head is not built in this engine."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError('SegmenterMaskTransformerAdapter (the Segmenter semantic-segmentation head) is not built in '
                                  'multimae_amd; use ConvNeXtAdapter (--output_adapter convnext)')
