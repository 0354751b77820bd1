"""TinyCLIP's learnable pruning masks — host-side mirror of TinyCLIP/src/open_clip/l0module.py:11-353 (`L0Module`, after
CoFiPruning): hard-concrete masks over the hidden dimension (`hidden_z`, one per tower), the heads (`heads_z`, per layer),
the MLP's intermediate units (`intermediate_z`, per layer) and — pruning type `layer` — whole attention / MLP branches
(`mha_z`, `ffn_z`), with the Lagrangian sparsity term of the automatic weight-inheritance recipe.

Same constructor arguments, parameter names (`hidden_loga`, `heads_loga`, `intermediate_loga`, `ffn_loga`, `mha_loga`,
`lambda_1`, `lambda_2`), mask shapes (`shapes[...]`) and sequence of random draws in `_sample_z` (one `uniform_` per mask
type, in `pruning_type` order), so a CPU seed reproduces the reference's masks.  Host code only: the masks are tensors of
weight size at the most; what they do to the towers is in cream_amd.tinyclip.model / native.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


class L0Module(nn.Module):
    limit_a, limit_b, epsilon = -.1, 1.1, 1e-6
    all_types = ["hidden_z", "heads_z", "mha_z", "intermediate_z", "ffn_z"]

    def __init__(self, config, start_sparsity=0.0, target_sparsity=0.0, lagrangian_warmup=0, init_loga=0.5, temperature=2. / 3.,
                 pruning_type=("hidden", "heads", "intermediate", "layer"), magical_number=0.8):
        super().__init__()
        self.magical_number, self.lagrangian_warmup = magical_number, lagrangian_warmup
        self.pruning_type = list(pruning_type)
        self.start_sparsity, self.target_sparsity, self.temperature = start_sparsity, target_sparsity, temperature

        self.hidden_size, self.intermediate_size = config.hidden_size, config.intermediate_size
        self.num_attention_heads, self.num_hidden_layers = config.num_attention_heads, config.num_hidden_layers
        self.dim_per_head = self.hidden_size // self.num_attention_heads

        D, F_ = self.hidden_size, self.intermediate_size
        self.params_per_head_layer = D * D * 4 + D * 4
        self.params_per_head = self.params_per_head_layer // self.num_attention_heads
        self.params_per_mlp_layer = D * F_ * 2 + D + F_
        self.params_per_intermediate_dim = self.params_per_mlp_layer // F_
        # (the normalisation layers are not counted, l0module.py:48)
        self.full_model_size = (self.params_per_head_layer + self.params_per_mlp_layer) * self.num_hidden_layers
        self.prunable_model_size = 0

        init_loga = init_loga if isinstance(init_loga, float) else 0.5
        self.loga_mean = math.log(1.0 - self.epsilon - init_loga) - math.log(init_loga + self.epsilon)

        self.types, self.z_logas, self.parameters_per_dim, self.sizes, self.shapes = [], {}, {}, {}, {}
        self.hidden_loga = None
        self.hidden_type = None
        for t in self.pruning_type:
            self.initialize_one_module(t)
        self.lambda_1 = nn.Parameter(torch.tensor(10.00))
        self.lambda_2 = nn.Parameter(torch.tensor(10.00))

    def initialize_parameters(self, size, num_layer=None, mean=None):
        loga = nn.Parameter(torch.empty(num_layer, size) if num_layer is not None else torch.empty(size))
        loga.data.normal_(mean or self.loga_mean, 0)                # std 0 (l0module.py:79), but the generator advances as there
        return loga

    def initialize_one_module(self, module_name):
        L, D, F_, H = self.num_hidden_layers, self.hidden_size, self.intermediate_size, self.num_attention_heads
        default_mean = 10
        if module_name == "intermediate":
            self.intermediate_loga = self.initialize_parameters(F_, L, mean=default_mean)
            self.add_one_module(self.intermediate_loga, "intermediate", self.params_per_intermediate_dim, F_, [L, 1, 1, F_])
            self.prunable_model_size += self.params_per_mlp_layer * L
        elif module_name == "heads":
            self.heads_loga = self.initialize_parameters(H, L, mean=default_mean)
            self.add_one_module(self.heads_loga, "heads", self.params_per_head, H, [L, 1, H, 1, 1])
            self.prunable_model_size += self.params_per_head * L * H
        elif module_name == "hidden":
            self.hidden_loga = self.initialize_parameters(D, mean=default_mean)
            self.add_one_module(self.hidden_loga, "hidden", D * 4 + D * 4 * 2, D, [D])
        elif module_name == "layer":
            self.ffn_loga = self.initialize_parameters(L, mean=default_mean)
            self.add_one_module(self.ffn_loga, "ffn", self.params_per_mlp_layer, 1, [L])
            self.mha_loga = self.initialize_parameters(L, mean=default_mean)
            self.add_one_module(self.mha_loga, "mha", self.params_per_head * H, 1, [L])

    def add_one_module(self, z_loga, type_name, parameter_per_dim, size, shape):
        self.types.append(type_name)
        self.z_logas[type_name] = z_loga
        self.parameters_per_dim[type_name] = parameter_per_dim
        self.sizes[type_name] = size
        self.shapes[type_name] = shape

    def constrain_parameters(self):
        for key in self.z_logas:
            self.z_logas[key].data.clamp_(min=math.log(1e-2), max=math.log(1e2))

    def cdf_qz(self, x, loga):
        """CDF of the stretched concrete distribution at x."""
        xn = (x - self.limit_a) / (self.limit_b - self.limit_a)
        logits = math.log(xn) - math.log(1.0 - xn)
        return torch.sigmoid(logits * self.temperature - loga).clamp(min=self.epsilon, max=1 - self.epsilon)

    def score_loga(self, loga):
        return 1.0 - self.cdf_qz(0.0, loga)

    def get_num_parameters_and_constraint(self, hidden=False):
        num_parameters = 0
        layers, hidden_size, heads = self.num_hidden_layers, self.hidden_size, self.num_attention_heads
        device = self.z_logas[self.types[0]].device
        mha_score = self.score_loga(self.mha_loga).view(-1, 1, 1) if "mha" in self.types else torch.ones([layers, 1, 1]).to(device)
        heads_score = (self.score_loga(self.heads_loga).unsqueeze(dim=-1) if "heads" in self.types
                       else torch.ones([layers, heads, 1]).to(device))
        self.parameters_per_dim.setdefault("heads", self.params_per_head)
        self.parameters_per_dim.setdefault("intermediate", self.params_per_intermediate_dim)

        heads_score = heads_score * mha_score
        if hidden:
            hidden_score = self.score_loga(self.hidden_loga) if "hidden" in self.types else torch.ones([hidden_size]).to(device)
            num_parameters += torch.outer(hidden_score, heads_score.reshape(-1)).sum() * self.parameters_per_dim["heads"] / self.hidden_size
        else:
            num_parameters += heads_score.sum() * self.parameters_per_dim["heads"]

        ffn_score = self.score_loga(self.ffn_loga).unsqueeze(dim=-1) if "ffn" in self.types else 1
        intermediate_score = (self.score_loga(self.intermediate_loga) if "intermediate" in self.types
                              else torch.ones([layers, hidden_size * 4]).to(device))
        intermediate_score = intermediate_score * ffn_score
        if hidden:
            num_parameters += torch.sum(torch.outer(hidden_score, intermediate_score.reshape(-1))) * 2
        else:
            num_parameters += intermediate_score.sum() * self.parameters_per_dim["intermediate"]
        return num_parameters

    def get_target_sparsity(self, pruned_steps):
        return (self.target_sparsity - self.start_sparsity) * min(1, pruned_steps / self.lagrangian_warmup) + self.start_sparsity

    def lagrangian_regularization(self, pruned_steps):
        """-> (loss, expected sparsity as a float, target sparsity): one-sided — only too LITTLE sparsity is penalised."""
        target_sparsity = self.get_target_sparsity(pruned_steps) if self.lagrangian_warmup > 0 else self.target_sparsity
        expect_sparsity = 1 - self.get_num_parameters_and_constraint("hidden" in self.types) / self.prunable_model_size
        zero = torch.tensor(0.0, device=expect_sparsity.device)
        gap = torch.maximum(target_sparsity - expect_sparsity, zero)
        lagrangian_loss = self.lambda_1 * gap + self.lambda_2 * gap.square()
        return lagrangian_loss, expect_sparsity.detach().item(), target_sparsity

    def _sample_z(self, loga):                                          # training: one uniform draw of loga's shape
        u = torch.zeros_like(loga).uniform_(self.epsilon, 1.0 - self.epsilon)
        z = torch.sigmoid((torch.log(u) - torch.log(1 - u) + loga) / self.temperature)
        z = z * (self.limit_b - self.limit_a) + self.limit_a
        return F.hardtanh(z, min_val=0.0, max_val=1.0)

    def _deterministic_z(self, size, loga, soft=True):                  # inference
        soft_mask = torch.sigmoid(loga / self.temperature * self.magical_number)
        if not soft:
            return soft_mask
        num_zeros = round(size - self.score_loga(loga).sum().item())
        if num_zeros > 0:
            if soft_mask.ndim == 0:
                soft_mask = torch.tensor(0).to(loga.device)
            else:
                _, indices = torch.topk(soft_mask, k=num_zeros, largest=False)
                soft_mask[indices] = 0.
        return soft_mask

    def get_z_from_zs(self, zs):
        return {t: ((zs[t].squeeze().detach().cpu().numpy() > 0) if t in zs else np.ones(self.shapes[t])) for t in self.types}

    def calculate_model_size(self, zs):
        if zs is None:
            return {"pruned_sparsity": 0.0}
        layers, hidden_size, heads = self.num_hidden_layers, self.hidden_size, self.num_attention_heads
        nz = self.get_z_from_zs(zs)
        hidden_z = nz["hidden"] if "hidden" in nz else np.ones([hidden_size])
        heads_z = nz["heads"] if "heads" in nz else np.ones([layers, 1, heads, 1, 1])
        mha_z = nz["mha"].reshape(-1, 1, 1, 1, 1) if "mha" in nz else np.ones([heads_z.shape[0], 1, 1, 1, 1])
        intermediate_z = nz["intermediate"] if "intermediate" in nz else np.ones([layers, 1, 1, hidden_size * 4])
        ffn_z = nz["ffn"].reshape(-1, 1, 1, 1) if "ffn" in nz else np.ones([heads_z.shape[0], 1, 1, 1])

        remain_hidden = hidden_z.sum().item()
        remain_intermediate = intermediate_z.reshape(self.num_hidden_layers, self.intermediate_size).sum(-1).tolist()
        remain_heads = heads_z.reshape(self.num_hidden_layers, self.num_attention_heads).sum(-1).tolist()
        n_heads = np.outer((heads_z * mha_z).reshape(-1), hidden_z).sum().item()
        n_inter = np.outer((intermediate_z * ffn_z).reshape(-1), hidden_z).sum().item()
        remain_model_size = n_heads * self.dim_per_head * 4 + n_inter * 2
        pruned_model_size = self.prunable_model_size - remain_model_size
        return {
            'mha': mha_z.reshape(-1).astype(int).tolist(),
            'ffn': ffn_z.reshape(-1).astype(int).tolist(),
            'remain_hidden': remain_hidden,
            'remain_intermediate': remain_intermediate,
            'remain_heads': remain_heads,
            'pruned_params': pruned_model_size,
            'remain_params': remain_model_size,
            'pruned_sparsity': pruned_model_size / self.prunable_model_size,
        }

    def forward(self, soft=True):
        """-> {`<type>_z`: mask of shape `shapes[type]`}: a hard-concrete sample in training mode (differentiable in the
        log-alphas), the deterministic masks in eval mode (`soft`: the expected number of zeros is cut to exact 0)."""
        zs = {}
        if self.training:
            for t in self.types:
                zs[f"{t}_z"] = self._sample_z(self.z_logas[t]).reshape(self.shapes[t])
        else:
            for t in self.types:
                if t != "hidden":                                       # per layer
                    zs[f"{t}_z"] = torch.stack([self._deterministic_z(self.sizes[t], loga.detach(), soft=soft).reshape(self.shapes[t][1:])
                                                for loga in self.z_logas[t]])
                else:
                    zs[f"{t}_z"] = self._deterministic_z(self.sizes[t], self.hidden_loga.detach(), soft=soft)
        return zs

    @torch.no_grad()
    def l0_mask(self):
        zs = {}
        get_mask = lambda loga: torch.sigmoid(loga / self.temperature * self.magical_number)     # noqa: E731
        for t in self.types:
            if t == "hidden":
                zs[f"{t}_z"] = get_mask(self.hidden_loga)
            else:
                zs[f"{t}_z"] = torch.stack([get_mask(loga).reshape(self.shapes[t][1:]) for loga in self.z_logas[t]])
        return zs


__all__ = ["L0Module"]
