"""Generate the golden fixtures in tests/golden/ by RUNNING THE REFERENCE ITSELF
(imported read-only from /root/reference through tests/refshim.py) on seeded inputs.

    python tests/golden/make_golden.py            # needs /root/reference; CPU, ~2 min

The fixtures are small (digests, a few full tensors) and are committed; /root/reference
does not exist on the GPU box, so `-m gpu` tests, smoke() and bench.py only ever read
these files.  Weights are not stored: fixture_utils.fill_params regenerates them from
seeds on both sides.
"""
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import refshim  # noqa: E402
from fixture_utils import (SUBNET_S, SUBNET_T, SUPERNETS, fill_params, grad_digest, make_batch,  # noqa: E402
                           model_kwargs)

torch.set_num_threads(8)


def save(name, **arrays):
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}
    np.savez_compressed(os.path.join(HERE, name), **out)
    print(f"wrote {name}: {sum(a.nbytes for a in out.values()) / 1e3:.1f} kB")


def autoformer():
    ref = refshim.load_autoformer_reference()
    sample_configs = refshim.reference_sample_configs()
    kat = {}
    # --- parameter-count KATs (README 5.8M / 22.9M / 53.7M) and supernet totals
    for size, sub in (('T', SUBNET_T), ('S', SUBNET_S)):
        m = ref.Vision_TransformerSuper(**model_kwargs(size))
        kat[f'subnet_{size}_params'] = int(m.get_sampled_params_numel(sub))
        kat[f'supernet_{size}_params'] = int(sum(p.numel() for p in m.parameters()))
        kat[f'supernet_{size}_state_keys'] = sorted(m.state_dict().keys())
        kat[f'supernet_{size}_complexity'] = float(m.get_complexity(196))
        # golden sample_configs draws: random.seed(epoch) discipline of supernet_engine.py:36
        for epoch in (0, 1, 7):
            random.seed(epoch)
            kat[f'draws_{size}_epoch{epoch}'] = [sample_configs(SUPERNETS[size]['choices']) for _ in range(3)]
    mB = ref.Vision_TransformerSuper(**model_kwargs('B'))
    kat['supernet_B_params'] = int(sum(p.numel() for p in mB.parameters()))
    # --- relative index tables of RelativePosition2D_super at N=197
    rp = ref.RelativePosition2D_super(64, 14)
    rp.set_sample_config(64)
    with torch.no_grad():
        rp.embeddings_table_v.copy_(torch.arange(30).float().view(30, 1).expand(30, 64))
        rp.embeddings_table_h.zero_()
        fv = rp(197, 197)[..., 0].long()
        rp.embeddings_table_h.copy_(torch.arange(30).float().view(30, 1).expand(30, 64))
        rp.embeddings_table_v.zero_()
        fh = rp(197, 197)[..., 0].long()
    kat['rel_index_sum_v'] = int(fv.sum())
    kat['rel_index_sum_h'] = int(fh.sum())
    save('autoformer_rel_index.npz', iv=fv.to(torch.uint8), ih=fh.to(torch.uint8))
    json.dump(kat, open(os.path.join(HERE, 'autoformer_kat.json'), 'w'), indent=1)
    print("wrote autoformer_kat.json")

    # --- one full step (fwd + bwd, fp32, dropout/drop-path 0) per supernet size
    for size, batch, cfg in (('T', 2, None), ('S', 1, SUBNET_S)):
        torch.manual_seed(0)
        m = ref.Vision_TransformerSuper(**model_kwargs(size))
        fill_params(m, seed=3)
        if cfg is None:
            random.seed(0)
            cfg = sample_configs(SUPERNETS[size]['choices'])     # supernet-T: depth 13, E=216
        m.set_sample_config(cfg)
        m.train()
        images, target = make_batch(batch, seed=5)
        logits = m(images)
        loss = torch.sum(-target * torch.log_softmax(logits, dim=-1), dim=-1).mean()
        loss.backward()
        grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in m.named_parameters()}
        full = {}
        for k in ('cls_token', 'head.bias', 'norm.weight', 'blocks.0.attn.qkv.bias',
                  'blocks.0.attn.rel_pos_embed_k.embeddings_table_v', 'blocks.0.attn.rel_pos_embed_k.embeddings_table_h',
                  'blocks.0.attn.rel_pos_embed_v.embeddings_table_v', 'blocks.0.attn.rel_pos_embed_v.embeddings_table_h',
                  f'blocks.{cfg["layer_num"] - 1}.attn.rel_pos_embed_k.embeddings_table_h',
                  f'blocks.{cfg["layer_num"] - 1}.fc1.bias'):
            full['full|' + k] = grads[k]
        save(f'autoformer_{size}_step.npz', logits=logits, loss=loss.reshape(1),
             config=np.frombuffer(json.dumps(cfg).encode(), dtype=np.uint8), **grad_digest(grads), **full)

    # --- AttentionSuper alone (awkward widths: in 216, 3 heads of the super 4)
    torch.manual_seed(0)
    att = ref.AttentionSuper(256, num_heads=4, qkv_bias=True, relative_position=True, change_qkv=True,
                             max_relative_position=14)
    fill_params(att, seed=11)
    att.set_sample_config(sample_q_embed_dim=192, sample_num_heads=3, sample_in_embed_dim=216)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 197, 216, generator=g, requires_grad=True)
    gy = torch.randn(2, 197, 216, generator=g)
    y = att(x)
    y.backward(gy)
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in att.named_parameters()}
    save('autoformer_attention.npz', y=y, dx=x.grad,
         **{'full|' + k: v for k, v in grads.items() if 'embeddings_table' in k or k.endswith('bias')},
         **grad_digest(grads))


def irpe():
    irpe = refshim.load_irpe_reference(with_dropin=False)
    # --- bucket id tables (int, must be bit-exact).  (method, ratio, H, W, skip)
    cases = [('product', 1.9, 14, 14, 1), ('product', 1.9, 24, 24, 1), ('product', 1.9, 7, 10, 0),
             ('euc', 20, 14, 14, 1), ('euc', 1.9, 9, 5, 2), ('quant', 51, 14, 14, 1), ('quant', 1.9, 6, 6, 0),
             ('cross_rows', 56, 14, 14, 1), ('cross_cols', 56, 14, 14, 1), ('cross_rows', 1.9, 5, 8, 0),
             ('product', 3.0, 12, 12, 1), ('euc', 7.5, 24, 24, 1)]
    meth = dict(product=irpe.METHOD.PRODUCT, euc=irpe.METHOD.EUCLIDEAN, quant=irpe.METHOD.QUANT,
                cross_rows=irpe.METHOD.CROSS_ROWS, cross_cols=irpe.METHOD.CROSS_COLS)
    out, meta = {}, []
    for (name, ratio, h, w, skip) in cases:
        alpha, beta, gamma = 1 * ratio, 2 * ratio, 8 * ratio
        ids, nb = irpe.get_bucket_ids_2d(meth[name], h, w, skip, alpha, beta, gamma, dtype=torch.long)
        key = f'{name}_{ratio}_{h}x{w}_s{skip}'
        ids = ids.numpy()
        meta.append(dict(key=key, method=name, ratio=ratio, h=h, w=w, skip=skip, num_buckets=int(nb),
                         sum=int(ids.sum()), shape=list(ids.shape)))
        if ids.shape[0] <= 200:
            out[key] = ids.astype(np.uint8 if nb < 256 else np.int16)
        else:   # 577x577: keep the checksum plus every 16th row
            out[key + '|rows16'] = ids[::16].astype(np.uint8)
    # piecewise_index on a dense integer and float grid (rounding-sensitive: half-to-even, float beta clip)
    xs = torch.arange(-64, 65)
    for ratio in (1.9, 3.0, 7.5, 20, 51):
        out[f'piecewise_int_{ratio}'] = irpe.piecewise_index(xs, ratio, 2 * ratio, 8 * ratio, torch.long).numpy().astype(np.int16)
        xf = torch.arange(0, 400).float().sqrt().round()
        out[f'piecewise_flt_{ratio}'] = irpe.piecewise_index(xf, ratio, 2 * ratio, 8 * ratio, torch.long).numpy().astype(np.int16)
    json.dump(meta, open(os.path.join(HERE, 'irpe_buckets.json'), 'w'), indent=1)
    save('irpe_buckets.npz', **out)

    # --- iRPE modules: forward + grads, contextual {q,k}:transposed, v:non-transposed, bias mode
    outs = {}
    for tag, kw in (('ctx_shared', dict(mode='ctx', shared_head=True)), ('ctx_perhead', dict(mode='ctx', shared_head=False)),
                    ('bias_perhead', dict(mode='bias', shared_head=False))):
        rpe_on = 'qkv' if kw['mode'] == 'ctx' else 'qk'
        cfg = irpe.get_rpe_config(ratio=1.9, method='product', skip=1, rpe_on=rpe_on, **kw)
        mods = irpe.build_rpe(cfg, head_dim=64, num_heads=3)
        g = torch.Generator().manual_seed(31)
        for which, mod in zip('qkv', mods):
            if mod is None:
                continue
            with torch.no_grad():
                for p in mod.parameters():
                    p.copy_(0.3 * torch.randn(p.shape, generator=g))
            if which == 'v':
                x = torch.randn(2, 3, 197, 197, generator=g).softmax(-1).requires_grad_()
            else:
                x = torch.randn(2, 3, 197, 64, generator=g, requires_grad=True)
            y = mod(x)
            gy = torch.randn(y.shape, generator=g)
            grads = torch.autograd.grad(y, [x] + list(mod.parameters()), gy, allow_unused=True)
            outs[f'{tag}|{which}|y'] = y[:, :, ::7, ::5] if y.shape[-1] == 197 else y[:, :, ::7]
            outs[f'{tag}|{which}|ysum'] = y.double().sum().reshape(1)
            if grads[0] is not None:
                outs[f'{tag}|{which}|dx'] = grads[0][:, :, ::7, ::5] if grads[0].shape[-1] == 197 else grads[0][:, :, ::7]
                outs[f'{tag}|{which}|dxsum'] = grads[0].double().sum().reshape(1)
            outs[f'{tag}|{which}|dw'] = grads[1]
    save('irpe_modules.npz', **outs)

    # --- RPEAttention + DeiT-tiny iRPE-K (BASELINE config 1): single image forward on CPU
    irpe2, rvt, models, rpe_models = refshim.load_irpe_models()
    torch.manual_seed(0)
    model = rpe_models.deit_tiny_patch16_224_ctx_product_50_shared_k()
    fill_params(model, seed=17)
    model.eval()
    x = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        logits = model(x)
    save('deit_tiny_irpe_k.npz', logits=logits, n_params=np.array([sum(p.numel() for p in model.parameters())]))
    # RPEAttention fwd/bwd, rpe on q, k and v
    cfg = irpe2.get_rpe_config(ratio=1.9, method='product', mode='ctx', shared_head=True, skip=1, rpe_on='qkv')
    att = rvt.RPEAttention(192, num_heads=3, qkv_bias=True, rpe_config=cfg)
    fill_params(att, seed=19)
    with torch.no_grad():
        for n, p in att.named_parameters():
            if 'lookup_table' in n:
                p.copy_(0.3 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n))))
    g = torch.Generator().manual_seed(41)
    x = torch.randn(2, 197, 192, generator=g, requires_grad=True)
    gy = torch.randn(2, 197, 192, generator=g)
    y = att(x)
    y.backward(gy)
    grads = {k: p.grad for k, p in att.named_parameters()}
    save('irpe_attention.npz', y=y, dx=x.grad, **{'full|' + k: v for k, v in grads.items() if 'lookup' in k or k.endswith('bias')},
         **grad_digest(grads))


def irpe_ext():
    """Round-2 fixtures (VERDICT r1 #1c, #5): the rest of the iRPE family the way the reference's other
    callers use it — bias mode (shared / per head), euclidean / quant / cross methods, skip = 0 and
    non-square maps (DETR-with-iRPE/models/transformer.py:49-69, rpe_attention_function.py:328-376) —
    and RPEAttention at the DeiT-base-384 sequence length L = 577 (BASELINE config 4 geometry)."""
    irpe = refshim.load_irpe_reference(with_dropin=False)
    outs = {}
    cases = [
        ('bias_shared', dict(ratio=1.9, method='product', mode='bias', shared_head=True, skip=1, rpe_on='qk'), 3, 14, 14),
        ('euc_ctx', dict(ratio=1.9, method='euc', mode='ctx', shared_head=True, skip=1, rpe_on='qkv'), 3, 14, 14),
        ('quant_ctx', dict(ratio=1.9, method='quant', mode='ctx', shared_head=False, skip=1, rpe_on='qkv'), 2, 14, 14),
        ('cross_ctx', dict(ratio=1.9, method='cross', mode='ctx', shared_head=True, skip=1, rpe_on='qkv'), 2, 14, 14),
        ('cross_bias', dict(ratio=1.9, method='cross', mode='bias', shared_head=False, skip=1, rpe_on='k'), 2, 14, 14),
        ('skip0_rect', dict(ratio=1.9, method='product', mode='ctx', shared_head=True, skip=0, rpe_on='qkv'), 2, 10, 14),
        ('skip0_rect_bias', dict(ratio=1.9, method='product', mode='bias', shared_head=False, skip=0, rpe_on='k'), 2, 9, 5),
    ]
    meta = []
    for tag, kw, heads, h, w in cases:
        cfg = irpe.get_rpe_config(**kw)
        mods = irpe.build_rpe(cfg, head_dim=64, num_heads=heads)
        L = h * w + kw['skip']
        g = torch.Generator().manual_seed(zlib_seed(tag))
        meta.append(dict(tag=tag, kw=kw, heads=heads, h=h, w=w, L=L))
        for which, mod in zip('qkv', mods):
            if mod is None:
                continue
            with torch.no_grad():
                for p in mod.parameters():
                    p.copy_(0.3 * torch.randn(p.shape, generator=g))
            if which == 'v':
                x = torch.randn(2, heads, L, L, generator=g).softmax(-1).requires_grad_()
            else:
                x = torch.randn(2, heads, L, 64, generator=g, requires_grad=True)
            y = mod(x, height=h, width=w)
            gy = torch.randn(y.shape, generator=g)
            params = list(mod.parameters())
            grads = torch.autograd.grad(y, [x] + params, gy, allow_unused=True)
            sub = (lambda t: t[:, :, ::7, ::5] if (t.shape[-1] == L and L > 150) else t)    # keep the files small
            outs[f'{tag}|{which}|y'] = sub(y)
            outs[f'{tag}|{which}|ysum'] = y.double().sum().reshape(1)
            if grads[0] is not None:
                outs[f'{tag}|{which}|dx'] = sub(grads[0])
            for i, gp in enumerate(grads[1:]):
                outs[f'{tag}|{which}|dw{i}'] = gp
    json.dump(meta, open(os.path.join(HERE, 'irpe_modules_ext.json'), 'w'), indent=1)
    save('irpe_modules_ext.npz', **outs)

    # RPEAttention at L = 577 (24 x 24 + class token), 3 heads of 64, rpe on k and on q, k, v
    irpe2, rvt, models, rpe_models = refshim.load_irpe_models()
    outs = {}
    for rpe_on in ('k', 'qkv'):
        cfg = irpe2.get_rpe_config(ratio=1.9, method='product', mode='ctx', shared_head=True, skip=1, rpe_on=rpe_on)
        att = rvt.RPEAttention(192, num_heads=3, qkv_bias=True, rpe_config=cfg)
        fill_params(att, seed=29)
        with torch.no_grad():
            for n, p in att.named_parameters():
                if 'lookup_table' in n:
                    p.copy_(0.3 * torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n) + 5)))
        g = torch.Generator().manual_seed(43)
        x = torch.randn(1, 577, 192, generator=g, requires_grad=True)
        gy = torch.randn(1, 577, 192, generator=g)
        y = att(x)
        y.backward(gy)
        grads = {k: p.grad for k, p in att.named_parameters()}
        outs[f'{rpe_on}|y'] = y[:, ::3]
        outs[f'{rpe_on}|dx'] = x.grad[:, ::3]
        for k, v in grads.items():
            if 'lookup' in k or k.endswith('bias'):
                outs[f'{rpe_on}|full|{k}'] = v
        for k, v in grad_digest(grads).items():
            outs[f'{rpe_on}|{k}'] = v
    save('irpe_attention_L577.npz', **outs)


def zlib_seed(tag):
    import zlib
    return zlib.crc32(tag.encode()) & 0x7fffffff


def autoformer_trace():
    """The boundary as the reference's UNCHANGED caller drives it: every call that
    model/supernet_transformer.py makes into `model.module.*` while it builds AutoFormer-T, applies a
    sampled configuration and runs one forward — class, constructor arguments, set_sample_config
    arguments, forward input shapes, in order.  The GPU box has no reference checkout: there the
    test replays OUR caller (cream_amd/autoformer/supernet.py) under the same recorder and requires the
    identical trace, then checks the numbers of the same step against autoformer_T_step.npz."""
    import cream_amd.dropin as d
    from cream_amd.dropin import trace as T
    refshim._install_torch_six()
    try:
        d.install_autoformer(os.path.join(refshim.AUTOFORMER, 'model'))
        import importlib
        st = importlib.import_module('model.supernet_transformer')
        assert st.__file__.startswith('/root/reference/')
        rec = T.Recorder()
        with rec.patch(st):
            m = st.Vision_TransformerSuper(**model_kwargs('T'))
            cfg = json.loads(bytes(np.load(os.path.join(HERE, 'autoformer_T_step.npz'))['config']).decode())
            m.set_sample_config(cfg)
            m.train()
            images, target = make_batch(2, seed=5)
            m(images)
        json.dump(rec.events, open(os.path.join(HERE, 'autoformer_call_trace.json'), 'w'))
        print(f'wrote autoformer_call_trace.json: {len(rec.events)} boundary calls')
    finally:
        for k in [k for k in sys.modules if k == 'model' or k.startswith('model.')]:
            del sys.modules[k]
        if d.PATH in sys.path:
            sys.path.remove(d.PATH)


def fake_accuracy(config, which):
    """Deterministic stand-in for an evaluation pass: a function of the candidate only."""
    import zlib
    key = repr((config['layer_num'], [float(x) for x in config['mlp_ratio']], [int(x) for x in config['num_heads']],
                int(config['embed_dim'][0]), which))
    return (zlib.crc32(key.encode()) % 100000) / 1000.0


def evolution():
    """AutoFormer/evolution.py's own EvolutionSearcher (class source executed from the read-only file,
    its timm / dataset imports left out) driven for two generations with a stubbed evaluator: the visited
    candidates, populations and top lists are the fixture the host-side mirror must reproduce."""
    import ast
    import tempfile
    import types
    ref = refshim.load_autoformer_reference()
    src = open(os.path.join(refshim.AUTOFORMER, 'evolution.py')).read()
    tree = ast.parse(src)
    keep = [n for n in tree.body if (isinstance(n, ast.FunctionDef) and n.name == 'decode_cand_tuple') or
            (isinstance(n, ast.ClassDef) and n.name == 'EvolutionSearcher')]
    visited = []

    def evaluate(loader, model, device, amp=True, mode='retrain', retrain_config=None):
        acc = fake_accuracy(retrain_config, loader)
        if loader == 'val':
            visited.append(retrain_config)
        return {'acc1': acc}

    ns = {'random': random, 'torch': torch, 'os': os, 'np': np, 'evaluate': evaluate,
          'utils': types.SimpleNamespace(get_rank=lambda: 0), 'print': lambda *a, **k: None}
    exec(compile(ast.Module(body=keep, type_ignores=[]), 'evolution.py', 'exec'), ns)
    model = ref.Vision_TransformerSuper(**model_kwargs('S'))
    args = types.SimpleNamespace(max_epochs=2, select_num=4, population_num=10, m_prob=0.2, s_prob=0.4, crossover_num=4,
                                 mutation_num=4, param_limits=23, min_param_limits=18, resume='', amp=True)
    with tempfile.TemporaryDirectory() as tmp:
        es = ns['EvolutionSearcher'](args, 'cpu', model, model, SUPERNETS['S']['choices'], 'val', 'test', tmp)
        random.seed(0)
        es.search()
    out = dict(args=vars(args), memory=es.memory, top50=es.keep_top_k[50], top_select=es.keep_top_k[4],
               candidates=es.candidates, top_accuracies=es.top_accuracies,
               visited=[[c['layer_num'], c['mlp_ratio'], c['num_heads'], c['embed_dim'][0]] for c in visited],
               params={repr(k): v.get('params') for k, v in es.vis_dict.items() if 'params' in v})
    json.dump(out, open(os.path.join(HERE, 'evolution_trace.json'), 'w'))
    print(f"wrote evolution_trace.json: {len(visited)} evaluated candidates, {len(es.vis_dict)} seen")


def tinyclip_loss():
    """TinyCLIP/src/open_clip/clip_soft_loss.py's ClipSoftLoss (class source executed from the read-only
    file together with loss.py's gather_feature; their open_clip / horovod imports left out) at world size 1
    on seeded features: loss and feature gradients."""
    import ast
    tc = os.path.join(refshim.REFERENCE, 'TinyCLIP', 'src', 'open_clip')
    ns = {'torch': torch, 'nn': torch.nn, 'F': torch.nn.functional, 'dist': torch.distributed, 'hvd': None,
          'nullcontext': __import__('contextlib').nullcontext, 'np': np}
    for fname, names in (('loss.py', ('gather_feature',)), ('clip_soft_loss.py', ('ClipSoftLoss',))):
        tree = ast.parse(open(os.path.join(tc, fname)).read())
        keep = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
        exec(compile(ast.Module(body=keep, type_ignores=[]), fname, 'exec'), ns)
    g = torch.Generator().manual_seed(77)
    feats = [torch.nn.functional.normalize(torch.randn(24, 64, generator=g), dim=-1).requires_grad_(i < 2) for i in range(4)]
    loss_fn = ns['ClipSoftLoss'](local_loss=True, gather_with_grad=False, rank=0, world_size=1)
    # world size 1: gather_feature's all_gather of one tensor is the identity; run it without a process group
    ns['dist'] = type('D', (), {'all_gather': staticmethod(lambda outs, x: outs[0].copy_(x))})
    ns['gather_feature'].__globals__['dist'] = ns['dist']
    out = {}
    for avg in (True, False):
        for f in feats[:2]:
            f.grad = None
        res = loss_fn(feats[0], feats[1], torch.tensor(50.0), feats[2], feats[3], torch.tensor(100.0), average_two_losses=avg)
        tot = res if avg else res[0] + 2 * res[1]
        tot.backward()
        out[f'avg{int(avg)}|loss'] = torch.stack(list(res)) if not avg else res.reshape(1)
        out[f'avg{int(avg)}|dimage'] = feats[0].grad.clone()
        out[f'avg{int(avg)}|dtext'] = feats[1].grad.clone()
    save('tinyclip_soft_loss.npz', **out)


DETR_CASES = {
    # --enc_rpe2d rpe-2.0-product-ctx-1-k (the DETR-with-iRPE README's recipe), padded images in the batch
    'product_k_padmask': dict(kw=dict(ratio=2.0, method='product', mode='ctx', shared_head=True, skip=0, rpe_on='k'), hw=(10, 14),
                              mask='pad'),
    'euc_qkv_addmask': dict(kw=dict(ratio=1.9, method='euc', mode='ctx', shared_head=False, skip=0, rpe_on='qkv'), hw=(9, 5),
                              mask='add'),
    'quant_bias_qk': dict(kw=dict(ratio=1.9, method='quant', mode='bias', shared_head=True, skip=0, rpe_on='qk'), hw=(6, 11),
                          mask=None),
}


def detr_inputs(tag, c, embed=256, batch=2):
    h, w = c['hw']
    L = h * w
    g = torch.Generator().manual_seed(zlib_seed(tag))
    src, pos, gy = (torch.randn(L, batch, embed, generator=g) for _ in range(3))
    pad = add = None
    if c['mask'] == 'pad':                      # the right part / bottom rows of image 1 are padding
        m = torch.zeros(batch, h, w, dtype=torch.bool)
        m[1, :, w - 3:] = True
        m[1, h - 2:, :] = True
        pad = m.flatten(1)
    elif c['mask'] == 'add':
        add = 0.5 * torch.randn(L, L, generator=g)
    return src, pos, gy, pad, add


def detr_fill(att, seed):
    with torch.no_grad():
        for n, p in att.named_parameters():
            g = torch.Generator().manual_seed(zlib_seed(n) ^ seed)
            p.copy_((0.3 if 'lookup_table' in n else (0.05 if p.dim() == 1 else p.shape[-1] ** -0.5)) * torch.randn(p.shape, generator=g))


def detr():
    """DETR-with-iRPE's encoder self-attention (models/rpe_attention/multi_head_attention.py): q = k = src + pos, v = src
    (models/transformer.py encoder layer), rectangular maps, key padding / additive masks, head_dim 32."""
    irpe, mha = refshim.load_detr_rpe_attention()
    import contextlib
    import io
    outs = {}
    for tag, c in DETR_CASES.items():
        with contextlib.redirect_stdout(io.StringIO()):          # the constructor prints the bucket counts
            att = mha.RPEMultiheadAttention(256, 8, dropout=0.0, rpe_config=irpe.get_rpe_config(**c['kw']))
        detr_fill(att, seed=31)
        src, pos, gy, pad, add = detr_inputs(tag, c)
        src.requires_grad_()
        pos.requires_grad_()
        qk = src + pos
        out, wts = att(qk, qk, src, key_padding_mask=pad, attn_mask=add, hw=c['hw'])
        (out * gy).sum().backward()
        for name, t in (('out', out), ('dsrc', src.grad), ('dpos', pos.grad)):          # strided sample + norm (file size)
            outs[f'{tag}|{name}'] = t[::6, :, ::2]
            outs[f'{tag}|{name}|norm'] = t.double().norm().reshape(1)
        outs[f'{tag}|weights'] = wts[:, ::5, ::3]
        for n, p in att.named_parameters():
            outs[f'{tag}|grad|{n}'] = p.grad if ('lookup' in n or p.dim() == 1) else p.grad[::5, ::3]
        outs[f'{tag}|keys'] = np.frombuffer(json.dumps(list(att.state_dict().keys())).encode(), dtype=np.uint8)
    save('detr_rpe_attention.npz', **outs)


def tinyclip_ckpt_layouts(keys):
    """The layouts a CLIP checkpoint is found in, built from the new-layout key list."""
    new = {k: i for i, k in enumerate(keys)}
    ddp = {'.'.join(k.split('.')[:1] + ['module'] + k.split('.')[1:]): v for k, v in new.items()}
    old = {}
    for k, v in new.items():
        head, rest = k.split('.', 1)
        old[rest if head != '_logit_scale' else 'logit_scale'] = v
    old_ddp = {'module.' + k: v for k, v in old.items()}
    return dict(new=new, new_from_ddp=ddp, old=old, old_under_module=old_ddp)


def tinyclip_ckpt():
    """open_clip/model.py convert_to_new_checkpoint(used_ddp=False) + the `.module` strip of CLIPBase.load_state_dict on
    the four layouts: resulting key -> value id."""
    m = refshim.load_tinyclip_model()
    c = TINYCLIP_CASES['small_quickgelu']
    model = m.CLIP(c['embed_dim'], dict(c['vision_cfg']), dict(c['text_cfg']), quick_gelu=True)
    keys = list(model.state_dict().keys())
    out = {}
    for name, sd in tinyclip_ckpt_layouts(keys).items():
        conv = m.convert_to_new_checkpoint(dict(sd), False)
        conv = {k.replace('.module', ''): v for k, v in conv.items()}                   # CLIPBase.load_state_dict :1066-1070
        out[name] = conv
    json.dump(dict(keys=keys, converted=out), open(os.path.join(HERE, 'tinyclip_ckpt.json'), 'w'))


RASAMPLER_CASES = [(1000, 1, 0, 0, True), (1000, 4, 3, 5, True), (777, 8, 2, 1, True), (513, 3, 1, 7, False), (256, 2, 1, 2, True),
                   (300, 7, 6, 3, True), (5000, 8, 0, 11, True)]          # (dataset length, replicas, rank, epoch, shuffle)


def rasampler():
    """AutoFormer/lib/samplers.py RASampler: the index sequences of a few (length, replicas, rank, epoch) combinations."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('_ref_samplers', os.path.join(refshim.AUTOFORMER, 'lib', 'samplers.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = []
    for n, R, r, ep, sh in RASAMPLER_CASES:
        s = mod.RASampler(range(n), num_replicas=R, rank=r, shuffle=sh)
        s.set_epoch(ep)
        out.append(dict(case=[n, R, r, ep, sh], len=len(s), indices=list(iter(s))))
    json.dump(out, open(os.path.join(HERE, 'rasampler.json'), 'w'))


TINYCLIP_CASES = {
    # BASELINE config 5's student (model_configs/TinyCLIP-ViT-39M-16-Text-19M.json)
    'vit39m16_text19m': dict(embed_dim=512, vision_cfg=dict(image_size=224, layers=12, width=512, patch_size=16),
                             text_cfg=dict(context_length=77, vocab_size=49408, width=512, heads=8, layers=6), quick_gelu=False),
    # OpenAI-style activation, 128-wide model with 64-wide heads, shorter context
    'small_quickgelu': dict(embed_dim=64, vision_cfg=dict(image_size=64, layers=2, width=128, patch_size=16),
                            text_cfg=dict(context_length=20, vocab_size=300, width=128, heads=2, layers=2), quick_gelu=True),
}


TINYCLIP_STRIDE = 4999


def tinyclip_fill(model, seed):
    with torch.no_grad():
        for n, p in model.named_parameters():
            g = torch.Generator().manual_seed(zlib_seed(n) ^ seed)
            if n.endswith('logit_scale'):
                continue
            if 'ln_' in n and n.endswith('weight'):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
            elif 'embedding' in n:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            else:
                fan_in = p.shape[1] if p.dim() == 2 else p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) * fan_in ** -0.5)


def tinyclip_inputs(tag, c, batch=2):
    g = torch.Generator().manual_seed(zlib_seed(tag))
    size, ctx, vocab = c['vision_cfg']['image_size'], c['text_cfg']['context_length'], c['text_cfg']['vocab_size']
    images = torch.randn(batch, 3, size, size, generator=g)
    texts = torch.randint(1, vocab - 1, (batch, ctx), generator=g)
    for b in range(batch):                          # the end-of-text token has the highest id; padding after it is 0
        eot = int(torch.randint(3, ctx, (1,), generator=g))
        texts[b, eot] = vocab - 1
        texts[b, eot + 1:] = 0
    gi = torch.randn(batch, c['embed_dim'], generator=g)
    gt = torch.randn(batch, c['embed_dim'], generator=g)
    return images, texts, gi, gt


def tinyclip_model():
    """TinyCLIP's CLIP class (open_clip/model.py) on seeded weights and inputs: normalised image / text features, logit
    scale and the gradient of every parameter (the towers of BASELINE config 5)."""
    m = refshim.load_tinyclip_model()
    outs, meta = {}, {}
    for tag, c in TINYCLIP_CASES.items():
        torch.manual_seed(0)
        model = m.CLIP(c['embed_dim'], dict(c['vision_cfg']), dict(c['text_cfg']), quick_gelu=c['quick_gelu'])
        tinyclip_fill(model, seed=37)
        images, texts, gi, gt = tinyclip_inputs(tag, c)
        fi, ft, scale = model(images, texts, normalized=True)
        ((fi * gi).sum() + (ft * gt).sum() + scale).backward()
        grads = {k: p.grad for k, p in model.named_parameters()}
        assert all(v is not None for v in grads.values())
        meta[tag] = dict(keys=list(model.state_dict().keys()), n_params=sum(p.numel() for p in model.parameters()))
        outs[f'{tag}|image_features'] = fi
        outs[f'{tag}|text_features'] = ft
        outs[f'{tag}|scale'] = scale.reshape(1)
        for k, v in grad_digest(grads, stride=TINYCLIP_STRIDE).items():
            outs[f'{tag}|{k}'] = v
    json.dump(meta, open(os.path.join(HERE, 'tinyclip_model.json'), 'w'), indent=1)
    save('tinyclip_model.npz', **outs)


MINIVIT_CASES = {
    # the registered model (mini_deit_models.py:23-30): no class token, rpe on k, two repeats, head transforms
    'mini_deit_tiny': dict(registered=True),
    # the same machinery without head transforms, rpe on q, k, v, class token: the configuration the fused iRPE
    # attention covers
    'shared_qkv_cls': dict(registered=False, depth=4, repeated_times=2, use_transform=False, use_cls_token=True, rpe_on='qkv',
                           skip=1, drop_path_rate=0.0),
}


def minivit_fill(model, seed):
    fill_params(model, seed=seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            g = torch.Generator().manual_seed(zlib_seed(n) ^ seed)
            if 'lookup_table' in n:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            elif 'norm' in n and n.endswith('weight'):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))


def minivit():
    """MiniViT/Mini-DeiT (weight-shared DeiT, per-repeat iRPE / norms / head transforms): logits and gradients of the
    reference's own model classes on seeded weights and inputs (the RepeatedModuleList use)."""
    from functools import partial
    irpe, mvt, models, mini = refshim.load_minivit_models()
    outs, meta = {}, {}
    for tag, c in MINIVIT_CASES.items():
        torch.manual_seed(0)
        if c['registered']:
            # = mini_deit_tiny_patch16_224() (mini_deit_models.py:9-30), whose lazy `from irpe import ...` needs the
            # reference directory on sys.path at call time
            cfg = irpe.get_rpe_config(ratio=1.9, method='product', mode='ctx', shared_head=True, skip=0, rpe_on='k')
            model = models.deit_tiny_patch16_224(rpe_config=cfg, use_cls_token=False, repeated_times=2, use_transform=True)
        else:
            cfg = irpe.get_rpe_config(ratio=1.9, method='product', mode='ctx', shared_head=True, skip=c['skip'], rpe_on=c['rpe_on'])
            model = mvt.VisionTransformer(patch_size=16, embed_dim=192, depth=c['depth'], num_heads=3, mlp_ratio=4, qkv_bias=True,
                                          norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), rpe_config=cfg,
                                          use_cls_token=c['use_cls_token'], repeated_times=c['repeated_times'],
                                          use_transform=c['use_transform'], drop_path_rate=c['drop_path_rate'])
        minivit_fill(model, seed=23)
        model.eval()
        g = torch.Generator().manual_seed(zlib_seed(tag))
        x = torch.randn(2, 3, 224, 224, generator=g)
        gy = torch.randn(2, 1000, generator=g)
        logits = model(x)
        (logits * gy).sum().backward()
        grads = {k: p.grad for k, p in model.named_parameters()}
        assert all(v is not None for v in grads.values())
        meta[tag] = dict(keys=list(model.state_dict().keys()), n_params=sum(p.numel() for p in model.parameters()))
        outs[f'{tag}|logits'] = logits
        for k, v in grad_digest(grads).items():
            outs[f'{tag}|{k}'] = v
    json.dump(meta, open(os.path.join(HERE, 'minivit.json'), 'w'), indent=1)
    save('minivit.npz', **outs)


def irpe_zoo():
    """The six checkpoints the reference's model zoo provides (rpe_models.py:10-19): state-dict keys, shapes and
    parameter counts of the registered constructors that load them (rpe_models.py:48-193) — what a published
    `<name>.pth` ({'model': state_dict}) must fit into."""
    irpe2, rvt, models, rpe_models = refshim.load_irpe_models()
    meta = {}
    for name in sorted(rpe_models._provided_checkpoints):
        model = getattr(rpe_models, name)()
        sd = model.state_dict()
        meta[name] = dict(keys=list(sd.keys()), shapes=[list(v.shape) for v in sd.values()],
                          n_params=sum(p.numel() for p in model.parameters()))
    json.dump(meta, open(os.path.join(HERE, 'irpe_zoo.json'), 'w'))
    print('irpe_zoo.json', {k: v['n_params'] for k, v in meta.items()})


def rpe_index_ref():
    """Digests of what the reference's own compiled operator (oracle/build_ref.py -> oracle/_ref) returns on the inputs of
    tests/test_rpe_index_cpu.py::test_oracle_matches_compiled_reference: forward_cpu and, single-threaded, backward_cpu."""
    from fixture_utils import RPE_INDEX_REF_CASES, digest, rpe_index_ref_inputs
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), 'oracle'))
    import build_ref
    build_ref.build()
    ref = build_ref.load_ref()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)           # the reference's accumulation order is only defined single-threaded
    cases = []
    for case, (nb, x, index, g) in zip(RPE_INDEX_REF_CASES, rpe_index_ref_inputs()):
        rec = dict(case=list(case[:5]) + [str(case[5])], x=digest(x), index=digest(index), y=digest(ref.forward_cpu(x, index)))
        if g is not None:
            gin = torch.zeros(x.shape, dtype=x.dtype)
            ref.backward_cpu(gin, g, index)
            rec.update(g=digest(g), gin=digest(gin))
        cases.append(rec)
    torch.set_num_threads(threads)
    json.dump(dict(cases=cases), open(os.path.join(HERE, 'rpe_index_ref.json'), 'w'), indent=1)
    print('rpe_index_ref.json', len(cases), 'cases')


if __name__ == '__main__':
    assert refshim.have_reference(), "needs the reference checkout at /root/reference"
    which = sys.argv[1:] or ['autoformer', 'irpe']
    if 'autoformer' in which:
        autoformer()
    if 'irpe' in which:
        irpe()
    if 'irpe_ext' in which:
        irpe_ext()
    if 'autoformer_trace' in which:
        autoformer_trace()
    if 'evolution' in which:
        evolution()
    if 'tinyclip_loss' in which:
        tinyclip_loss()
    if 'minivit' in which:
        minivit()
    if 'detr' in which:
        detr()
    if 'tinyclip_model' in which:
        tinyclip_model()
    if 'rasampler' in which:
        rasampler()
    if 'tinyclip_ckpt' in which:
        tinyclip_ckpt()
    if 'irpe_zoo' in which:
        irpe_zoo()
    if 'rpe_index_ref' in which:
        rpe_index_ref()
