"""The cross-modality building blocks of the sibling model (unsupervised_visualbert/src/lxrt/modeling.py) on the HIP
kernels -- SURVEY 8f / N4, last part.  Same class names, constructor arguments, forward signatures and state-dict keys:

  BertAttention(config, ctx_dim=None)   :349-404   query from hidden_states, key / value from `context` (any width ctx_dim)
  BertAttOutput                         :406-417   dense -> dropout -> LayerNorm(x + input)
  BertCrossattLayer / BertSelfattLayer  :420-443
  BertIntermediate / BertOutput         :445-471
  LXRTXLayer                            :667-717   cross-attention in both directions with ONE shared BertCrossattLayer,
                                                   self-attention per modality, FFN per modality
  VisualFeatEncoder                     :719-767   (LayerNorm(visn_fc(feats)) + LayerNorm(box_fc(boxes))) / 2, dropout

Every FLOP runs in libvisualbert_hip.so: the Linears through vb_gemm (ops.LinearFn), dropout + residual + LayerNorm through
vb_ln_fwd / vb_ln_bwd (ops.LayerNormFn), the attention core through vb_attn_cross_fwd / vb_attn_cross_bwd
(ops.CrossAttentionCoreFn: queries and keys / values from different sequences of different lengths, scores never in HBM).
These are stand-alone modules (no flat parameter arena): gradients reach `.grad` through autograd as usual.

  LXRTEncoder                           :769-905   VisualFeatEncoder + either (visualbert_style) a stack of BertLayer over the
                                                   concatenated [language; vision] sequence, or the l / r / x stack: BertLayer
                                                   over the language, BertLayer over the regions, LXRTXLayer across both

The reference's own constructor reaches the l / r / x stack only through an `assert(0)` (lxrt/modeling.py:803-804): no
argument set builds it there, but its forward (:893-905) is well defined, and tests/golden/base_lxrt_encoder.npz pins this
class against that forward run on the reference's own blocks (the golden generator assembles the module around the assert).  `output_attention` (returning the probabilities) is not offered: NotImplementedError, never silent.

  BertVisualObjHead                     :971-996   transform + one decoder per visual loss, into ONE score buffer
  LXRTPretrainingHeads                  :1297-1420 the heads of LXRTPretraining (`cls`, `obj_predict_head`) and its loss lines:
                                                   masked LM, image-text match and the masked-region objective -- object class,
                                                   attribute class, feature regression per region, each weighted by a per-region
                                                   confidence / mask -- through ops.VisualLossFn (vb_visual_loss_fwd_bwd)
  BertVisualAnswerHead                  :956-969   Linear(H, 2H) -> GeLU -> LayerNorm(2H) -> Linear(2H, num_answers): GELU +
                                                   LayerNorm in one kernel over the wide rows (ops.WideLayerNormFn), the VQA /
                                                   GQA fine-tuning loss on its fp32 logits (ops.BCELogitsLossFn)
  LXRTPretrainingHeadsQA                :1327-1436 LXRTPretrainingHeads + `answer_head` and the `qa` term (task_qa)"""
import torch
from torch import nn

from . import ops
from .modeling import BertConfig, BertLayer, BertLayerNorm  # noqa: F401  (re-exported: the reference module defines them too)


def _p(drop, training):
    return float(drop.p) if training else 0.0


def _mask_add(attention_mask, B, Sk, device):
    """the reference hands an ADDITIVE mask broadcastable to [B, heads, Sq, Sk] (extended attention mask, (1 - m) * -10000);
    the kernels take fp32 [B, Sk] over the keys."""
    if attention_mask is None:
        return torch.zeros((B, Sk), dtype=torch.float32, device=device)
    m = attention_mask.to(torch.float32)
    if m.numel() != B * Sk:
        raise NotImplementedError("attention_mask must broadcast over heads and queries ([B, 1, 1, Sk]); got %s" % (tuple(m.shape),))
    return m.reshape(B, Sk).contiguous()


class BertAttention(nn.Module):
    _next_sid = [64]                      # dropout stream ids of these stand-alone blocks (the encoder layers use 8 .. 8 + 8 L)

    def __init__(self, config, ctx_dim=None):
        super(BertAttention, self).__init__()
        if config.hidden_size % config.num_attention_heads != 0:
            raise ValueError("The hidden size (%d) is not a multiple of the number of attention heads (%d)"
                             % (config.hidden_size, config.num_attention_heads))
        self.num_attention_heads = config.num_attention_heads
        self.attention_head_size = int(config.hidden_size / config.num_attention_heads)
        if self.attention_head_size != 64:
            raise NotImplementedError("attention kernels are built for head size 64 (BERT-base 768 / 12)")
        self.all_head_size = self.num_attention_heads * self.attention_head_size
        if ctx_dim is None:
            ctx_dim = config.hidden_size
        self.query = nn.Linear(config.hidden_size, self.all_head_size)
        self.key = nn.Linear(ctx_dim, self.all_head_size)
        self.value = nn.Linear(ctx_dim, self.all_head_size)
        self.dropout = nn.Dropout(config.attention_probs_dropout_prob)
        self._sid = BertAttention._next_sid[0]
        BertAttention._next_sid[0] += 4

    def forward(self, hidden_states, context, attention_mask=None):
        B, Sk = context.size(0), context.size(1)
        q = ops.LinearFn.apply(hidden_states, self.query.weight, self.query.bias, None, False)
        k = ops.LinearFn.apply(context, self.key.weight, self.key.bias, None, False)
        v = ops.LinearFn.apply(context, self.value.weight, self.value.bias, None, False)
        mask_add = _mask_add(attention_mask, B, Sk, hidden_states.device)
        return ops.CrossAttentionCoreFn.apply(q, k, v, mask_add, self.num_attention_heads, _p(self.dropout, self.training),
                                              self._sid)


class BertAttOutput(nn.Module):
    def __init__(self, config):
        super(BertAttOutput, self).__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        self._sid = BertAttention._next_sid[0]
        BertAttention._next_sid[0] += 4

    def forward(self, hidden_states, input_tensor):
        h = ops.LinearFn.apply(hidden_states, self.dense.weight, self.dense.bias, None, False)
        return ops.LayerNormFn.apply(h, input_tensor, self.LayerNorm.weight, self.LayerNorm.bias,
                                     self.LayerNorm.variance_epsilon, _p(self.dropout, self.training), 0.0, self._sid)


class BertCrossattLayer(nn.Module):
    def __init__(self, config):
        super(BertCrossattLayer, self).__init__()
        self.att = BertAttention(config)
        self.output = BertAttOutput(config)

    def forward(self, input_tensor, ctx_tensor, ctx_att_mask=None):
        output = self.att(input_tensor, ctx_tensor, ctx_att_mask)
        return self.output(output, input_tensor)


class BertSelfattLayer(nn.Module):
    def __init__(self, config):
        super(BertSelfattLayer, self).__init__()
        self.self = BertAttention(config)
        self.output = BertAttOutput(config)

    def forward(self, input_tensor, attention_mask):
        self_output = self.self(input_tensor, input_tensor, attention_mask)      # keys and queries are the same tensor
        return self.output(self_output, input_tensor)


class BertIntermediate(nn.Module):
    def __init__(self, config):
        super(BertIntermediate, self).__init__()
        self.dense = nn.Linear(config.hidden_size, config.intermediate_size)
        if config.hidden_act != "gelu":
            raise NotImplementedError("hidden_act %r: the fused epilogue implements BERT's erf-GELU" % (config.hidden_act,))

    def forward(self, hidden_states):
        return ops.LinearFn.apply(hidden_states, self.dense.weight, self.dense.bias, "gelu", False)


class BertOutput(nn.Module):
    def __init__(self, config):
        super(BertOutput, self).__init__()
        self.dense = nn.Linear(config.intermediate_size, config.hidden_size)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        self._sid = BertAttention._next_sid[0]
        BertAttention._next_sid[0] += 4

    def forward(self, hidden_states, input_tensor):
        h = ops.LinearFn.apply(hidden_states, self.dense.weight, self.dense.bias, None, False)
        return ops.LayerNormFn.apply(h, input_tensor, self.LayerNorm.weight, self.LayerNorm.bias,
                                     self.LayerNorm.variance_epsilon, _p(self.dropout, self.training), 0.0, self._sid)


class LXRTXLayer(nn.Module):
    def __init__(self, config):
        super(LXRTXLayer, self).__init__()
        self.visual_attention = BertCrossattLayer(config)          # ONE set of weights for both directions (:665, :680-681)
        self.lang_self_att = BertSelfattLayer(config)
        self.visn_self_att = BertSelfattLayer(config)
        self.lang_inter = BertIntermediate(config)
        self.lang_output = BertOutput(config)
        self.visn_inter = BertIntermediate(config)
        self.visn_output = BertOutput(config)

    def cross_att(self, lang_input, lang_attention_mask, visn_input, visn_attention_mask):
        lang_att_output = self.visual_attention(lang_input, visn_input, ctx_att_mask=visn_attention_mask)
        visn_att_output = self.visual_attention(visn_input, lang_input, ctx_att_mask=lang_attention_mask)
        return lang_att_output, visn_att_output

    def self_att(self, lang_input, lang_attention_mask, visn_input, visn_attention_mask):
        return self.lang_self_att(lang_input, lang_attention_mask), self.visn_self_att(visn_input, visn_attention_mask)

    def output_fc(self, lang_input, visn_input):
        lang_output = self.lang_output(self.lang_inter(lang_input), lang_input)
        visn_output = self.visn_output(self.visn_inter(visn_input), visn_input)
        return lang_output, visn_output

    def forward(self, lang_feats, lang_attention_mask, visn_feats, visn_attention_mask):
        lang_att_output, visn_att_output = self.cross_att(lang_feats, lang_attention_mask, visn_feats, visn_attention_mask)
        lang_att_output, visn_att_output = self.self_att(lang_att_output, lang_attention_mask, visn_att_output,
                                                         visn_attention_mask)
        return self.output_fc(lang_att_output, visn_att_output)


class VisualFeatEncoder(nn.Module):
    def __init__(self, config, visual_feat_dim=2048, visual_pos_dim=4):
        """the reference reads the two widths from its global VISUAL_CONFIG (:718-719); here they are arguments."""
        super(VisualFeatEncoder, self).__init__()
        self.visn_fc = nn.Linear(visual_feat_dim, config.hidden_size)
        self.visn_layer_norm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.box_fc = nn.Linear(visual_pos_dim, config.hidden_size)
        self.box_layer_norm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        self._sid = BertAttention._next_sid[0]
        BertAttention._next_sid[0] += 4

    def forward(self, visn_input):
        feats, boxes = visn_input
        dt = feats.dtype
        x = ops.LinearFn.apply(feats, self.visn_fc.weight, self.visn_fc.bias, None, False)
        x = ops.LayerNormFn.apply(x, None, self.visn_layer_norm.weight, self.visn_layer_norm.bias,
                                  self.visn_layer_norm.variance_epsilon, 0.0, 0.0, self._sid)
        # box_fc has K = 4: below the GEMM kernels' 8-element operand granularity -> the box matrix is zero-padded to 8 columns
        # (exact: the padded products are zeros)
        Bq, R, P = boxes.shape
        pad = (-P) % 8
        bx, w = boxes.to(dt), self.box_fc.weight
        if pad:
            bx = torch.nn.functional.pad(bx, (0, pad))
            w = _PadColumns.apply(w, pad)
        y = ops.LinearFn.apply(bx, w, self.box_fc.bias, None, False)
        y = ops.LayerNormFn.apply(y, None, self.box_layer_norm.weight, self.box_layer_norm.bias,
                                  self.box_layer_norm.variance_epsilon, 0.0, 0.0, self._sid + 1)
        out = (x + y) * 0.5
        p = _p(self.dropout, self.training)
        return ops.DropoutFn.apply(out, p, self._sid + 2) if p > 0.0 else out


def _cat_with_none(a, b, dim):
    if a is None:
        return b
    if b is None:
        return a
    return torch.cat((a, b), dim=dim)


class LXRTEncoder(nn.Module):
    """lxrt/modeling.py:769-905.  The reference reads the layer counts and `visualbert_style` from globals (VISUAL_CONFIG /
    args); here they are constructor arguments.  forward(lang_feats, lang_attention_mask, visn_feats, visn_attention_mask):
    lang_feats [B, Tl, H] (the word embeddings are applied outside, :829-830), visn_feats = (features [B, R, Dv], boxes
    [B, R, 4]) or None, masks additive and broadcastable ([B, 1, 1, S], (1 - m) * -10000).  Returns (lang_feats, visn_feats).
    BertLayer is the fused encoder layer of visualbert_amd.modeling (same state-dict keys as the sibling's :719-731)."""

    def __init__(self, config, l_layers=12, x_layers=5, r_layers=0, visualbert_style=False, visual_feat_dim=2048,
                 visual_pos_dim=4):
        super(LXRTEncoder, self).__init__()
        self.visn_fc = VisualFeatEncoder(config, visual_feat_dim=visual_feat_dim, visual_pos_dim=visual_pos_dim)
        self.num_l_layers, self.num_x_layers, self.num_r_layers = l_layers, x_layers, r_layers
        self.visualbert_style = visualbert_style
        self.layer = nn.ModuleList([BertLayer(config) for _ in range(l_layers)])
        for i, m in enumerate(self.layer):                       # dropout stream ids of the fused layers: clear of the blocks'
            m.set_index(64 + i)
        if not visualbert_style:
            self.x_layers = nn.ModuleList([LXRTXLayer(config) for _ in range(x_layers)])
            self.r_layers = nn.ModuleList([BertLayer(config) for _ in range(r_layers)])
            for i, m in enumerate(self.r_layers):
                m.set_index(64 + l_layers + i)
        self.config = config

    def forward(self, lang_feats, lang_attention_mask, visn_feats, visn_attention_mask=None, layer_limit=-1):
        if visn_feats is not None and visn_feats[0] is not None:
            visn_feats = self.visn_fc(visn_feats)
        else:
            visn_feats = None
        if self.visualbert_style:                                # :853-891 (default switches)
            joint = _cat_with_none(lang_feats, visn_feats, dim=1)
            joint_mask = _cat_with_none(lang_attention_mask, visn_attention_mask, dim=-1)
            layers = self.layer if layer_limit == -1 else self.layer[:layer_limit]
            for layer_module in layers:
                joint = layer_module(joint, joint_mask)
            if lang_feats is None:
                return None, joint
            if visn_feats is None:
                return joint, None
            Tl = lang_feats.size(1)
            return joint[:, :Tl, :].contiguous(), joint[:, Tl:, :].contiguous()
        if lang_feats is not None:                               # :893-905
            for layer_module in self.layer:
                lang_feats = layer_module(lang_feats, lang_attention_mask)
        for layer_module in self.r_layers:
            visn_feats = layer_module(visn_feats, visn_attention_mask)
        if lang_feats is not None:
            for layer_module in self.x_layers:
                lang_feats, visn_feats = layer_module(lang_feats, lang_attention_mask, visn_feats, visn_attention_mask)
        return lang_feats, visn_feats


class _PadColumns(torch.autograd.Function):
    """[N, K] -> [N, K + pad] with zero columns, as a fresh fp32 leaf-like tensor the GEMM wrappers accept (they key bf16
    shadows on parameter identity); the gradient of the real columns flows back."""

    @staticmethod
    def forward(ctx, w, pad):
        ctx.k = w.size(1)
        return torch.nn.functional.pad(w.detach(), (0, pad)).contiguous()

    @staticmethod
    def backward(ctx, g):
        return g[:, :ctx.k].contiguous(), None


#: default output widths of the visual decoders: 1600 detector object classes, 400 attribute classes, the 2048-d region feature
#: (the reference's VISUAL_CONFIG.visual_loss_config)
VISUAL_LOSS_SIZES = {"obj": 1600, "attr": 400, "feat": 2048}


def _visual_loss_keys(visual_losses):
    keys = [k for k in str(visual_losses).split(",") if k]
    for k in keys:
        if k not in ops.VISUAL_SEGMENTS:
            raise NotImplementedError("visual loss %r: the objective kernel implements %s" % (k, ", ".join(ops.VISUAL_SEGMENTS)))
    if not keys or len(set(keys)) != len(keys):
        raise ValueError("visual_losses %r: one to three different keys of %s" % (visual_losses, ops.VISUAL_SEGMENTS))
    return keys


class BertVisualObjHead(nn.Module):
    """lxrt/modeling.py:971-996, same state-dict keys (transform.dense / transform.LayerNorm / decoder_dict.<key>).  The
    reference reads the decoder widths from its global VISUAL_CONFIG; here they are an argument (`sizes`, per key).

    forward(hidden_states [.., H]) returns ONE score buffer T [M, ld] (M = rows of hidden_states, ld a multiple of 64) instead
    of the reference's dict of three tensors: its column blocks are the decoders' outputs in the order ops.VISUAL_SEGMENTS
    (obj | attr | feat, absent keys left out; the default visual_losses order) -- the layout ops.VisualLossFn reads.
    `segment_widths()` gives (n_obj, n_attr, n_feat); `scores_dict(buffer)` the reference's dict as views."""

    def __init__(self, config, visual_losses="obj,attr,feat", sizes=None):
        super(BertVisualObjHead, self).__init__()
        from .modeling import BertPredictionHeadTransform
        self.transform = BertPredictionHeadTransform(config)
        self.visual_losses = _visual_loss_keys(visual_losses)
        sizes = dict(VISUAL_LOSS_SIZES if sizes is None else sizes)
        self.sizes = {k: int(sizes[k]) for k in self.visual_losses}
        for k, n in self.sizes.items():
            if n <= 0 or n % 8:
                raise NotImplementedError("decoder %r of width %d: column blocks of the score buffer start on 16-byte boundaries "
                                          "(widths are multiples of 8)" % (k, n))
        self.decoder_dict = nn.ModuleDict({k: nn.Linear(config.hidden_size, self.sizes[k]) for k in self.visual_losses})

    def segment_widths(self):
        return tuple(self.sizes.get(k, 0) for k in ops.VISUAL_SEGMENTS)

    def scores_dict(self, scores):
        out, off = {}, 0
        for k in ops.VISUAL_SEGMENTS:
            if k in self.sizes:
                out[k] = scores[:, off:off + self.sizes[k]]
                off += self.sizes[k]
        return out

    def forward(self, hidden_states):
        h = self.transform(hidden_states)
        segs = tuple(i for i, k in enumerate(ops.VISUAL_SEGMENTS) if k in self.sizes)
        params = []
        for i in segs:
            lin = self.decoder_dict[ops.VISUAL_SEGMENTS[i]]
            params += [lin.weight, lin.bias]
        return ops.VisualDecoderFn.apply(h, segs, *params)


class LXRTPretrainingHeads(nn.Module):
    """The heads and the loss lines of LXRTPretraining (lxrt/modeling.py:1297-1420) over the encoder's outputs: `cls` (masked LM
    with the decoder tied to `word_embedding_weight`, image-text match) and `obj_predict_head` (masked-region modelling), under
    the reference's attribute names.  forward returns (total_loss, losses [1, n], losses_dict) with the reference's terms, order
    and names: "Masked LM", "Matches", then the keys of visual_losses.  obj_labels: {key: (label, mask_conf)} -- int class ids
    [B, R] for obj / attr, the fp32 target feature [B, R, D] for feat, one confidence / mask per region.  Every visual term is
    (loss_r * mask_conf_r).mean() * loss_weight (the reference's 1 / 0.15; its `weight_disable` is loss_weight=1.0).
    The QA answer head (`task_qa`) is the subclass LXRTPretrainingHeadsQA, not a switch of this class.
    Not offered (NotImplementedError, never silently different): the tag / symbolic heads, lxmert_style_nlvr and the `kl`
    loss form."""

    def __init__(self, config, word_embedding_weight, task_mask_lm=True, task_matched=True, task_obj_predict=True,
                 visual_losses="obj,attr,feat", loss_weight=1 / 0.15, sizes=None, task_qa=False,
                 use_tag_symbolic_embedding=False, lxmert_style_nlvr=False, loss_forms=None):
        super(LXRTPretrainingHeads, self).__init__()
        from .modeling import BertPreTrainingHeads
        if task_qa:
            raise NotImplementedError("task_qa: the answer head and its `qa` term are LXRTPretrainingHeadsQA(config, "
                                      "word_embedding_weight, num_answers, ...), a subclass of this class")
        if use_tag_symbolic_embedding:
            raise NotImplementedError("use_tag_symbolic_embedding: the tag / symbolic heads are not implemented")
        if lxmert_style_nlvr:
            raise NotImplementedError("lxmert_style_nlvr is not implemented")
        forms = {"obj": "ce", "attr": "ce", "feat": "l2"}
        for k, f in (loss_forms or {}).items():
            if forms.get(k) != f:
                raise NotImplementedError("loss form %r for %r: the kernel implements ce for obj / attr and l2 for feat" % (f, k))
        self.task_mask_lm, self.task_matched, self.task_obj_predict = task_mask_lm, task_matched, task_obj_predict
        self.visual_losses = _visual_loss_keys(visual_losses)
        self.loss_weight = float(loss_weight)
        self.cls = BertPreTrainingHeads(config, word_embedding_weight)
        if task_obj_predict:
            self.obj_predict_head = BertVisualObjHead(config, visual_losses, sizes=sizes)

    def forward(self, lang_output, pooled_output, visn_output, masked_lm_labels=None, matched_label=None, obj_labels=None):
        return self._finish(*self._terms(lang_output, pooled_output, visn_output, masked_lm_labels, matched_label, obj_labels),
                            lang_output if lang_output is not None else visn_output)

    @staticmethod
    def _finish(total_loss, losses, losses_dict, like):
        if total_loss is None:
            total_loss = torch.zeros((), device=like.device)
        return total_loss, torch.stack(losses).unsqueeze(0) if losses else torch.zeros((1, 0)), losses_dict

    def _terms(self, lang_output, pooled_output, visn_output, masked_lm_labels, matched_label, obj_labels):
        """(total_loss or None, [terms, detached], {name: term, detached}) in the reference's order"""
        total_loss = None
        losses, losses_dict = [], {}

        def add(name, term):
            nonlocal total_loss
            total_loss = term if total_loss is None else total_loss + term
            losses.append(term.detach())
            losses_dict[name] = term.detach()

        if masked_lm_labels is not None and self.task_mask_lm:
            pred = self.cls.predictions
            tr = pred.transform
            _, mlm_loss = ops.MLMHeadLossFn.apply(lang_output, masked_lm_labels.contiguous(), pred, pred.decoder.weight, pred.bias,
                                                  tr.dense.weight, tr.dense.bias, tr.LayerNorm.weight, tr.LayerNorm.bias)
            add("Masked LM" if visn_output is not None else "Text Only Masked LM", mlm_loss)
        if matched_label is not None and self.task_matched and pooled_output is not None:
            _, matched_loss = ops.SmallLinearCEFn.apply(pooled_output, matched_label.reshape(-1), -1,
                                                        self.cls.seq_relationship.weight, self.cls.seq_relationship.bias)
            add("Matches", matched_loss)
        if obj_labels is not None and self.task_obj_predict:
            head = self.obj_predict_head
            scores = head(visn_output)
            n_obj, n_attr, n_feat = head.segment_widths()
            args = []
            for k in ops.VISUAL_SEGMENTS:
                args += list(obj_labels[k]) if k in head.sizes else [None, None]
            w = self.loss_weight
            visn = ops.VisualLossFn.apply(scores, n_obj, n_attr, n_feat, *args, w, w, w)
            for k in self.visual_losses:
                add(k, visn[ops.VISUAL_SEGMENTS.index(k)])
        return total_loss, losses, losses_dict


class GeLU(nn.Module):
    """lxrt/modeling.py:121-131: index 1 of BertVisualAnswerHead.logit_fc, parameter-free.  It holds the reference's place in the
    nn.Sequential (so that the state-dict keys are logit_fc.0 / .2 / .3); the head applies it inside the LayerNorm kernel."""

    def forward(self, x):
        raise RuntimeError("visualbert_amd: GeLU is fused into the LayerNorm behind it (ops.WideLayerNormFn); call the head")


class BertVisualAnswerHead(nn.Module):
    """lxrt/modeling.py:956-969, same state-dict keys: logit_fc = Sequential(Linear(H, 2H), GeLU, BertLayerNorm(2H),
    Linear(2H, num_answers)) -- the `task_qa` head of LXRTPretraining and, verbatim, VQAModel.logit_fc / GQAModel.logit_fc
    (src/tasks/vqa_model.py:28-34).  A plain GEMM for logit_fc.0, GELU + LayerNorm in one kernel over the 2H-wide rows
    (ops.WideLayerNormFn), a GEMM to fp32 logits.

    forward(pooled)              -> logits fp32 [.., num_answers]
    forward(pooled, target=t)    -> (logits, loss, score): BCEWithLogitsLoss()(logits, t) * num_answers on soft targets t
                                    [B, num_answers] and the mean VQA score of the argmax (src/tasks/vqa.py:72, :106-107, :114-117)
    forward(pooled, labels=ans)  -> (logits, loss): CrossEntropyLoss(ignore_index=-1), the pre-training `qa` term (:1423-1436)"""

    def __init__(self, config, num_answers):
        super(BertVisualAnswerHead, self).__init__()
        hid_dim = config.hidden_size
        if hid_dim % 4 or not 8 <= hid_dim * 2 <= 8192:
            raise NotImplementedError("hidden_size %d: the wide LayerNorm kernel takes 2 x hidden_size in 8 .. 8192, a multiple of 8"
                                      % hid_dim)
        self.num_answers = int(num_answers)
        self.logit_fc = nn.Sequential(
            nn.Linear(hid_dim, hid_dim * 2),
            GeLU(),
            BertLayerNorm(hid_dim * 2, eps=1e-12),
            nn.Linear(hid_dim * 2, self.num_answers),
        )

    def forward(self, hidden_states, target=None, labels=None):
        fc0, ln, fc3 = self.logit_fc[0], self.logit_fc[2], self.logit_fc[3]
        h = ops.LinearFn.apply(hidden_states, fc0.weight, fc0.bias, None, False)
        h = ops.WideLayerNormFn.apply(h, ln.weight, ln.bias, ln.variance_epsilon, "gelu")
        if target is not None and labels is not None:
            raise ValueError("BertVisualAnswerHead: soft targets (the VQA loss) or class labels (the pre-training term), not both")
        if target is not None:
            return ops.BCELogitsLossFn.apply(h, target, fc3.weight, fc3.bias)
        if labels is not None:
            return ops.AnswerCELossFn.apply(h, labels, fc3.weight, fc3.bias)
        return ops.LinearFn.apply(h, fc3.weight, fc3.bias, None, True)


class LXRTPretrainingHeadsQA(LXRTPretrainingHeads):
    """LXRTPretrainingHeads with `task_qa` (lxrt/modeling.py:1327-1328, :1361-1362, :1423-1436): `answer_head`
    (BertVisualAnswerHead over the pooled output) and the `qa` term, CrossEntropyLoss(ignore_index=-1) of the answer scores
    against `ans`, placed after the visual terms.  forward returns the reference's four values
    (total_loss, losses [1, n], answer_score.detach(), losses_dict); without `ans` the head still runs and no term is added."""

    def __init__(self, config, word_embedding_weight, num_answers, **kwargs):
        if kwargs.pop("task_qa", True) is not True:
            raise ValueError("LXRTPretrainingHeadsQA is the task_qa form; use LXRTPretrainingHeads without it")
        super(LXRTPretrainingHeadsQA, self).__init__(config, word_embedding_weight, **kwargs)
        self.task_qa = True
        self.num_answers = int(num_answers)
        self.answer_head = BertVisualAnswerHead(config, self.num_answers)

    def forward(self, lang_output, pooled_output, visn_output, masked_lm_labels=None, matched_label=None, obj_labels=None,
                ans=None):
        total_loss, losses, losses_dict = self._terms(lang_output, pooled_output, visn_output, masked_lm_labels, matched_label,
                                                      obj_labels)
        if ans is not None:
            answer_score, answer_loss = self.answer_head(pooled_output, labels=ans.reshape(-1))
            total_loss = answer_loss if total_loss is None else total_loss + answer_loss
            losses.append(answer_loss.detach())
            losses_dict["qa"] = answer_loss.detach()
        else:
            answer_score = self.answer_head(pooled_output)
        total_loss, losses, losses_dict = self._finish(total_loss, losses, losses_dict, pooled_output)
        return total_loss, losses, answer_score.detach(), losses_dict


def lxrt_init_weights(module, initializer_range=0.02):
    """BertPreTrainedModel.init_bert_weights of the sibling (:1105-1116): N(0, 0.02) Linear / Embedding weights, zero biases,
    LayerNorm (1, 0)."""
    if isinstance(module, (nn.Linear, nn.Embedding)):
        module.weight.data.normal_(mean=0.0, std=initializer_range)
    elif isinstance(module, BertLayerNorm):
        module.bias.data.zero_()
        module.weight.data.fill_(1.0)
    if isinstance(module, nn.Linear) and module.bias is not None:
        module.bias.data.zero_()

