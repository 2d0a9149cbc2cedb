"""RoBERTa, the frozen text encoder of `--fixed_language_model roberta-large` (utils/utils_train.py:194-222 get_fixed_language_model,
train.py:274-290, test.py:85-86), over the native kernels of csrc/roberta.hip: embedding + LayerNorm with RoBERTa's padding-aware
position ids, the post-LN encoder layer loop (bf16 GEMMs with the erf-GELU epilogue, key-length attention) and masked mean pooling
(utils/utils.py:53-59).  The host side reproduces transformers' byte-level BPE RobertaTokenizer and RobertaModel's state_dict keys.

Inference only (the reference runs this model under no_grad and never trains it).  Nothing here downloads: checkpoints and vocabulary
files are read from a local directory."""

import ctypes
import json
import os
from functools import lru_cache

import torch
from torch import nn

from . import _lib, ops
from .shadow import Cached

f32, bf16 = torch.float32, torch.bfloat16
BOS, PAD, EOS = 0, 1, 2  # <s>, <pad>, </s>
TOKENIZER_FILES = ('vocab.json', 'merges.txt')
MODEL_FILES = ('config.json', 'model.safetensors or pytorch_model.bin')


def _need_dir(path, files, what):
    if not (isinstance(path, (str, os.PathLike)) and os.path.isdir(path)):
        raise FileNotFoundError(f'{what}: {path!r} is not a local directory.  This package never downloads; give a directory that '
                                f'holds {", ".join(files)} (e.g. a copy of the hub repository roberta-large).')


# ---- tokenizer -------------------------------------------------------------------------------------------
@lru_cache()
def bytes_to_unicode():
    """GPT-2's reversible byte -> printable unicode map (the alphabet of the byte-level BPE)."""
    bs = list(range(ord('!'), ord('~') + 1)) + list(range(ord('¡'), ord('¬') + 1)) + list(range(ord('®'), ord('ÿ') + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, map(chr, cs)))


PRETOKENIZE = r"""'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"""


class RobertaTokenizer:
    """transformers' RobertaTokenizer (byte-level BPE, add_prefix_space=False): <s> = 0, <pad> = 1, </s> = 2; a sequence is
    <s> tokens </s>.  __call__ pads to the longest sequence of the batch (right padding) and truncates to max_length keeping </s>."""

    def __init__(self, vocab_file, merges_file):
        import regex
        with open(vocab_file, encoding='utf-8') as f:
            self.encoder = json.load(f)
        with open(merges_file, encoding='utf-8') as f:
            lines = f.read().split('\n')
        merges = [tuple(l.split()) for l in lines if l and not l.startswith('#version')]
        self.bpe_ranks = {m: i for i, m in enumerate(merges)}
        self.byte_encoder = bytes_to_unicode()
        self.pat = regex.compile(PRETOKENIZE)
        self.cache = {}
        for tok, i in (('<s>', BOS), ('<pad>', PAD), ('</s>', EOS)):
            if self.encoder.get(tok) != i:
                raise ValueError(f'vocab.json: {tok} must have id {i} (RoBERTa\'s special tokens), got {self.encoder.get(tok)}')
        self.unk_id = self.encoder.get('<unk>', 3)
        self.pad_token_id = PAD

    @classmethod
    def from_pretrained(cls, path, **kwargs):
        _need_dir(path, TOKENIZER_FILES, 'RobertaTokenizer.from_pretrained')
        return cls(os.path.join(path, 'vocab.json'), os.path.join(path, 'merges.txt'))

    def bpe(self, token):
        if token in self.cache:
            return self.cache[token]
        word = list(token)
        while len(word) > 1:
            pairs = {(word[i], word[i + 1]) for i in range(len(word) - 1)}
            best = min(pairs, key=lambda p: self.bpe_ranks.get(p, float('inf')))
            if best not in self.bpe_ranks:
                break
            out, i = [], 0
            while i < len(word):
                if i < len(word) - 1 and (word[i], word[i + 1]) == best:
                    out.append(word[i] + word[i + 1])
                    i += 2
                else:
                    out.append(word[i])
                    i += 1
            word = out
        self.cache[token] = word
        return word

    def encode_plain(self, text):
        """ids of the text without the special tokens"""
        ids = []
        for piece in self.pat.findall(text):
            mapped = ''.join(self.byte_encoder[b] for b in piece.encode('utf-8'))
            ids.extend(self.encoder.get(t, self.unk_id) for t in self.bpe(mapped))
        return ids

    def __call__(self, texts, return_tensors='pt', padding=True, truncation=True, max_length=None):
        if isinstance(texts, str):
            texts = [texts]
        if return_tensors not in ('pt', None):
            raise NotImplementedError(f'return_tensors={return_tensors!r}: only "pt"')
        seqs = []
        for t in texts:
            body = self.encode_plain(t)
            if truncation and max_length is not None:
                body = body[:max(0, max_length - 2)]
            seqs.append([BOS] + body + [EOS])
        L = max(len(s) for s in seqs) if seqs else 0
        if not padding and len({len(s) for s in seqs}) > 1:
            raise ValueError('sequences of different lengths need padding=True')
        ids = torch.full((len(seqs), L), PAD, dtype=torch.int64)
        mask = torch.zeros(len(seqs), L, dtype=torch.int64)
        for i, s in enumerate(seqs):
            ids[i, :len(s)] = torch.tensor(s, dtype=torch.int64)
            mask[i, :len(s)] = 1
        return {'input_ids': ids, 'attention_mask': mask}


# ---- model ----------------------------------------------------------------------------------------------
class _Holder(nn.Module):
    """Parameter container (no forward): gives parameters their transformers names."""


def _linear(out_f, in_f):
    h = _Holder()
    h.weight = nn.Parameter(torch.randn(out_f, in_f) * 0.02)
    h.bias = nn.Parameter(torch.zeros(out_f))
    return h


def _ln(e):
    h = _Holder()
    h.weight = nn.Parameter(torch.ones(e))
    h.bias = nn.Parameter(torch.zeros(e))
    return h


class RobertaConfig:
    """The fields of a transformers RobertaConfig (config.json) that the forward uses; roberta-large's values by default."""

    def __init__(self, vocab_size=50265, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
                 hidden_act='gelu', max_position_embeddings=514, type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1, **_):
        self.vocab_size, self.hidden_size, self.num_hidden_layers = vocab_size, hidden_size, num_hidden_layers
        self.num_attention_heads, self.intermediate_size, self.hidden_act = num_attention_heads, intermediate_size, hidden_act
        self.max_position_embeddings, self.type_vocab_size = max_position_embeddings, type_vocab_size
        self.layer_norm_eps, self.pad_token_id = layer_norm_eps, pad_token_id

    @classmethod
    def from_json(cls, path):
        with open(path) as f:
            return cls(**json.load(f))


class RobertaModelOutput(tuple):
    """(last_hidden_state,) with the attribute transformers' BaseModelOutputWithPoolingAndCrossAttentions gives it; [0] is what
    mean_pooling reads.  The pooler is not computed (the reference never uses it)."""

    @property
    def last_hidden_state(self):
        return self[0]


class RobertaModel(nn.Module):
    def __init__(self, config=None):
        super().__init__()
        c = config or RobertaConfig()
        if c.hidden_act != 'gelu':
            raise NotImplementedError(f'hidden_act {c.hidden_act!r}: the encoder kernels implement the exact (erf) GELU only')
        if c.hidden_size != 64 * c.num_attention_heads:
            raise NotImplementedError(f'hidden_size {c.hidden_size} with {c.num_attention_heads} heads: the attention kernels need head '
                                      'dimension 64')
        if c.hidden_size > 1024 or c.intermediate_size % 8:
            raise NotImplementedError(f'hidden_size {c.hidden_size} / intermediate_size {c.intermediate_size}: need <= 1024 / a multiple of 8')
        self.config = c
        E, F = c.hidden_size, c.intermediate_size
        self.embeddings = _Holder()
        self.embeddings.word_embeddings = _Holder()
        self.embeddings.word_embeddings.weight = nn.Parameter(torch.randn(c.vocab_size, E) * 0.02)
        self.embeddings.token_type_embeddings = _Holder()
        self.embeddings.token_type_embeddings.weight = nn.Parameter(torch.randn(c.type_vocab_size, E) * 0.02)
        self.embeddings.LayerNorm = _ln(E)
        self.embeddings.position_embeddings = _Holder()  # (registered last, as transformers' RobertaEmbeddings does)
        self.embeddings.position_embeddings.weight = nn.Parameter(torch.randn(c.max_position_embeddings, E) * 0.02)
        self.encoder = _Holder()
        self.encoder.layer = nn.ModuleList()
        for _ in range(c.num_hidden_layers):
            ly = _Holder()
            ly.attention = _Holder()
            ly.attention.self = _Holder()
            for n in ('query', 'key', 'value'):
                setattr(ly.attention.self, n, _linear(E, E))
            ly.attention.output = _Holder()
            ly.attention.output.dense = _linear(E, E)
            ly.attention.output.LayerNorm = _ln(E)
            ly.intermediate = _Holder()
            ly.intermediate.dense = _linear(F, E)
            ly.output = _Holder()
            ly.output.dense = _linear(E, F)
            ly.output.LayerNorm = _ln(E)
            self.encoder.layer.append(ly)
        self.pooler = _Holder()
        self.pooler.dense = _linear(E, E)  # kept for the checkpoint's keys; not computed
        self._shadow, self._scratch = Cached(self._shadow_sources, self._build_shadow), None

    # ---- checkpoints --------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, path, **kwargs):
        """config.json + model.safetensors (or pytorch_model.bin) of a local directory.  A `roberta.` prefix (the hub checkpoint of
        roberta-large is a RobertaForMaskedLM) is stripped and `lm_head.*` ignored.  Returns the model in eval mode, frozen."""
        _need_dir(path, MODEL_FILES, 'RobertaModel.from_pretrained')
        model = cls(RobertaConfig.from_json(os.path.join(path, 'config.json')))
        st, binf = os.path.join(path, 'model.safetensors'), os.path.join(path, 'pytorch_model.bin')
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        elif os.path.exists(binf):
            sd = torch.load(binf, map_location='cpu', weights_only=True)
        else:
            raise FileNotFoundError(f'{path}: neither model.safetensors nor pytorch_model.bin')
        model.load_checkpoint(sd)
        return model.requires_grad_(False).eval()

    def load_checkpoint(self, sd):
        own = {}
        for k, v in sd.items():
            if k.startswith('lm_head.'):
                continue
            k = k[len('roberta.'):] if k.startswith('roberta.') else k
            if k in ('embeddings.position_ids', 'embeddings.token_type_ids'):  # buffers older checkpoints carry
                continue
            own[k] = v.float()
        missing = set(self.state_dict()) - set(own)
        if missing <= {'pooler.dense.weight', 'pooler.dense.bias'}:  # (RobertaForMaskedLM has no pooler: keep the initial values)
            for k in missing:
                own[k] = self.state_dict()[k]
        self.load_state_dict(own)

    # ---- forward --------------------------------------------------------------------------------------------
    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, **kwargs):
        """input_ids [B, L] (right padded with <pad> = 1), attention_mask [B, L] (1 = real token; a prefix of each row) ->
        RobertaModelOutput whose [0] is last_hidden_state [B, L, hidden] fp32."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError('mmvid_amd RobertaModel is inference only: call it under torch.no_grad(), or freeze its parameters '
                               '(requires_grad_(False); from_pretrained does)')
        if token_type_ids is not None and bool((token_type_ids != 0).any()):
            raise NotImplementedError('token_type_ids other than 0 (RoBERTa has one token type)')
        if kwargs.get('inputs_embeds') is not None or kwargs.get('position_ids') is not None:
            raise NotImplementedError('inputs_embeds / position_ids: give input_ids (positions follow from the padding)')
        c = self.config
        dev = self.embeddings.word_embeddings.weight.device
        ids = ops._chk(input_ids.to(dev, torch.int64).contiguous(), torch.int64, 'input_ids')
        if ids.dim() != 2:
            raise ValueError(f'input_ids must be [B, L], got {tuple(ids.shape)}')
        B, L = ids.shape
        if L + c.pad_token_id >= c.max_position_embeddings:
            raise ValueError(f'sequence length {L} exceeds the {c.max_position_embeddings - c.pad_token_id - 1} positions of the model')
        mask = None
        if attention_mask is not None:
            mask = attention_mask.to(dev, torch.int64).contiguous()
            if tuple(mask.shape) != (B, L):
                raise ValueError(f'attention_mask {tuple(mask.shape)} does not match input_ids {(B, L)}')
        E, H, F = c.hidden_size, c.num_attention_heads, c.intermediate_size
        with torch.no_grad():
            x = torch.empty(B, L, E, device=dev, dtype=f32)
            xb = torch.empty(B, L, E, device=dev, dtype=bf16)
            key_len = torch.empty(B, device=dev, dtype=torch.int32)
            em = self.embeddings
            _lib.call('mmvid_roberta_embed', ops._p(ids), ops._p(mask), B, L, ops._p(em.word_embeddings.weight), c.vocab_size,
                      ops._p(em.position_embeddings.weight), c.max_position_embeddings, ops._p(em.token_type_embeddings.weight),
                      ops._p(em.LayerNorm.weight), ops._p(em.LayerNorm.bias), c.layer_norm_eps, E, c.pad_token_id, ops._p(x), ops._p(xb),
                      ops._p(key_len), ops._stream())
            cfg = _lib.PostLnCfg(B, L, E, H, F, c.num_hidden_layers, c.layer_norm_eps)
            layers, _keep = self._layer_structs()
            nbytes = ctypes.c_int64()
            _lib.call('mmvid_postln_encoder_workspace', ctypes.byref(cfg), ctypes.byref(nbytes))
            if self._scratch is None or self._scratch.device != dev or self._scratch.numel() < nbytes.value:
                self._scratch = torch.empty(nbytes.value, device=dev, dtype=torch.uint8)
            _lib.call('mmvid_postln_encoder_forward', ctypes.byref(cfg), layers, ops._p(key_len), ops._p(x), ops._p(xb), ops._p(x),
                      ops._p(self._scratch), ops._stream())
        return RobertaModelOutput((x, ))

    # ---- native plumbing --------------------------------------------------------------------------------------
    def _shadow_sources(self):
        return [p for ly in self.encoder.layer for p in (ly.attention.self.query.weight, ly.attention.self.key.weight,
                                                         ly.attention.self.value.weight, ly.attention.self.query.bias,
                                                         ly.attention.self.key.bias, ly.attention.self.value.bias,
                                                         ly.attention.output.dense.weight, ly.intermediate.dense.weight,
                                                         ly.output.dense.weight)]

    def _build_shadow(self):
        """bf16 GEMM operands (built once, and again only when a weight changes: self._shadow): per layer Q|K|V packed [3E, E] with
        its bias [3E] fp32, attention.output.dense, intermediate.dense, output.dense."""
        sh = []
        for ly in self.encoder.layer:
            s = ly.attention.self
            qkv_w = torch.cat([s.query.weight, s.key.weight, s.value.weight]).detach().contiguous()
            qkv_b = torch.cat([s.query.bias, s.key.bias, s.value.bias]).detach().float().contiguous()
            sh.append((ops.cast_bf16(qkv_w), qkv_b, ops.cast_bf16(ly.attention.output.dense.weight.detach().contiguous()),
                       ops.cast_bf16(ly.intermediate.dense.weight.detach().contiguous()),
                       ops.cast_bf16(ly.output.dense.weight.detach().contiguous())))
        return sh

    def _layer_structs(self):
        sh = self._shadow.get()
        arr = (_lib.PostLnLayer * len(self.encoder.layer))()
        keep = []

        def ptr(t):
            keep.append(t)
            return t.data_ptr()

        for i, ly in enumerate(self.encoder.layer):
            a, (qkv_w, qkv_b, out_w, fc_w, pj_w) = arr[i], sh[i]
            a.qkv_w, a.qkv_b = ptr(qkv_w), ptr(qkv_b)
            a.out_w, a.out_b = ptr(out_w), ptr(ly.attention.output.dense.bias)
            a.ln1_w, a.ln1_b = ptr(ly.attention.output.LayerNorm.weight), ptr(ly.attention.output.LayerNorm.bias)
            a.fc_w, a.fc_b = ptr(fc_w), ptr(ly.intermediate.dense.bias)
            a.pj_w, a.pj_b = ptr(pj_w), ptr(ly.output.dense.bias)
            a.ln2_w, a.ln2_b = ptr(ly.output.LayerNorm.weight), ptr(ly.output.LayerNorm.bias)
        return arr, keep


def mean_pooling(model_output, attention_mask):
    """utils/utils.py:53-59: the mean of the token features whose mask is non-zero -> [B, hidden] fp32 (on the pooling kernel)."""
    x = model_output[0]
    x = ops._chk(x.to(f32).contiguous(), f32, 'token embeddings')
    B, L, E = x.shape
    mask = attention_mask.to(x.device, torch.int64).contiguous()
    if tuple(mask.shape) != (B, L):
        raise ValueError(f'attention_mask {tuple(mask.shape)} does not match the token embeddings {(B, L)}')
    out = torch.empty(B, E, device=x.device, dtype=f32)
    _lib.call('mmvid_masked_mean_pool', ops._p(x), ops._p(mask), B, L, E, ops._p(out), ops._stream())
    return out


def get_fixed_language_model(args, path=None):
    """utils/utils_train.py:194-222 -> (tokenizer2, language_model, text_feature_dim, encode_text).  `path`: a local directory with
    config.json, model.safetensors / pytorch_model.bin, vocab.json and merges.txt; by default args.fixed_language_model when that
    is a directory.  The model is on the current cuda device, frozen, in eval mode."""
    name = args.fixed_language_model
    if path is None:
        if isinstance(name, (str, os.PathLike)) and os.path.isdir(name):
            path = name
        elif name != 'roberta-large':
            raise NotImplementedError(f'fixed_language_model {name!r}: only roberta-large (as the reference)')
    _need_dir(path, TOKENIZER_FILES + MODEL_FILES, f'fixed_language_model {name!r}')
    tokenizer2 = RobertaTokenizer.from_pretrained(path)
    language_model = RobertaModel.from_pretrained(path).cuda()
    text_feature_dim = language_model.config.hidden_size

    @torch.no_grad()
    def encode_text(descriptions, device='cuda'):
        encoded_input = tokenizer2(descriptions, return_tensors='pt', padding=True, truncation=True, max_length=args.text_seq_len)
        encoded_input = {'input_ids': encoded_input['input_ids'].to(device), 'attention_mask': encoded_input['attention_mask'].to(device)}
        output = language_model(**encoded_input)
        return mean_pooling(output, encoded_input['attention_mask'])

    return tokenizer2, language_model, text_feature_dim, encode_text
