"""TEST INFRASTRUCTURE -- plain-PyTorch (CPU, differentiable) restatement of the encode-process-decode
model, used only by tests/ and bench.py's cpu_baseline as the gradient oracle of the HIP backward.

Follows gnn_manip/models/epd_gnn.py:72-105 (MLP structure, LayerNorm / residual placement) with the
block semantics of DESIGN.md section 2 (e' = phi_e(cat[h_i, h_j, e]), agg_i = sum e', h' =
phi_v(cat[h, agg]); j = edge_index[0], i = edge_index[1]).  Parameters are a state_dict-style mapping
(keys ``encoder.phi_edge.0.weight`` ...), the same one oracle/epd_oracle.py:init_params produces.
The forward of this file is itself checked against the numpy oracle (tests/test_oracle_golden.py).
"""
import torch
import torch.nn.functional as F


def mlp(p, prefix, x, num_layers, norm, ln_eps=1e-5):
    """Linear ReLU [Linear ReLU]x(L-1) Linear [LayerNorm]  (epd_gnn.py:72-84)."""
    for l in range(num_layers):
        x = F.relu(F.linear(x, p[f"{prefix}.{2 * l}.weight"], p[f"{prefix}.{2 * l}.bias"]))
    k = 2 * num_layers
    x = F.linear(x, p[f"{prefix}.{k}.weight"], p[f"{prefix}.{k}.bias"])
    if norm:
        x = F.layer_norm(x, (x.shape[1],), p[f"{prefix}.{k + 1}.weight"], p[f"{prefix}.{k + 1}.bias"], ln_eps)
    return x


def epd_forward(p, nodes, edge_attr, edge_index, num_layers, m_steps, ln_eps=1e-5):
    """epd_gnn.py:86-105."""
    j, i = edge_index[0], edge_index[1]
    h = mlp(p, "encoder.phi_node", nodes, num_layers, True, ln_eps)
    e = mlp(p, "encoder.phi_edge", edge_attr, num_layers, True, ln_eps)
    for k in range(m_steps):
        e_new = mlp(p, f"processor.{k}.phi_edge", torch.cat((h[i], h[j], e), dim=1), num_layers, True, ln_eps)
        agg = torch.zeros_like(h).index_add_(0, i, e_new)
        h_new = mlp(p, f"processor.{k}.phi_node", torch.cat((h, agg), dim=1), num_layers, True, ln_eps)
        h, e = h + h_new, e + e_new
    return mlp(p, "decoder", h, num_layers, False)


def loss_and_grads(params_np, nodes, edge_attr, edge_index, target, num_layers, m_steps, dtype=torch.float64, ln_eps=1e-5):
    """L1 loss of train_dyn.py:65 (sum / N) and its gradient w.r.t. every parameter, on the CPU."""
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in params_np.items()}
    out = epd_forward(p, torch.tensor(nodes, dtype=dtype), torch.tensor(edge_attr, dtype=dtype),
                      torch.tensor(edge_index, dtype=torch.int64), num_layers, m_steps, ln_eps)
    loss = F.l1_loss(out, torch.tensor(target, dtype=dtype), reduction="sum") / out.shape[0]
    loss.backward()
    return out.detach().numpy(), float(loss.detach()), {k: v.grad.numpy() for k, v in p.items()}


def _mlp_taped(p, prefix, x, num_layers, norm, tape, ln_eps=1e-5):
    """mlp() that records every hidden pre-activation z and activation a = relu(z) (both keep their gradients)."""
    for l in range(num_layers):
        z = F.linear(x, p[f"{prefix}.{2 * l}.weight"], p[f"{prefix}.{2 * l}.bias"])
        x = F.relu(z)
        x.retain_grad()
        tape.append((z, x))
    k = 2 * num_layers
    x = F.linear(x, p[f"{prefix}.{k}.weight"], p[f"{prefix}.{k}.bias"])
    if norm:
        x = F.layer_norm(x, (x.shape[1],), p[f"{prefix}.{k + 1}.weight"], p[f"{prefix}.{k + 1}.bias"], ln_eps)
    return x


def epd_forward_taped(p, nodes, edge_attr, edge_index, num_layers, m_steps, tape, ln_eps=1e-5):
    """epd_forward that appends (z, a) of every hidden Linear to `tape`, in evaluation order: node encoder, edge encoder, per
    step edge then node MLP, decoder -- num_layers entries each."""
    j, i = edge_index[0], edge_index[1]
    h = _mlp_taped(p, "encoder.phi_node", nodes, num_layers, True, tape, ln_eps)
    e = _mlp_taped(p, "encoder.phi_edge", edge_attr, num_layers, True, tape, ln_eps)
    for k in range(m_steps):
        e_new = _mlp_taped(p, f"processor.{k}.phi_edge", torch.cat((h[i], h[j], e), dim=1), num_layers, True, tape, ln_eps)
        agg = torch.zeros_like(h).index_add_(0, i, e_new)
        h_new = _mlp_taped(p, f"processor.{k}.phi_node", torch.cat((h, agg), dim=1), num_layers, True, tape, ln_eps)
        h, e = h + h_new, e + e_new
    return _mlp_taped(p, "decoder", h, num_layers, False, tape)


def near_zero_units(tape, tau=1e-5, max_units=256):
    """The hidden units of a tape with |z| < tau * rms(z of its Linear), as sorted (|z| / rms, tape entry, flat index): the closest
    to zero first, at most max_units.  Empty entries and entries with rms == 0 have none."""
    units = []
    for t, (z, a) in enumerate(tape):
        if z.numel() == 0:
            continue
        zz = z.detach().flatten()
        rms = float(zz.pow(2).mean().sqrt())
        if rms <= 0.0:
            continue
        for q in torch.nonzero(zz.abs() < tau * rms).flatten().tolist():
            units.append((float(zz[q].abs()) / rms, t, q))
    units.sort()
    return units[:max_units]


def flip_bounds(tape, units, leaves):
    """Per element of every leaf, what toggling the ReLU derivative of each of `units` alone can change in d loss / d leaf (first
    order), absolute values summed over the units.  The loss has been backpropagated through the tape's graph (retain_graph=True),
    so a.grad is d loss / d a_u: what reaches a unit from above whether or not its derivative lets it through."""
    bounds = [torch.zeros_like(v) for v in leaves]
    for _, t, q in units:
        z, a = tape[t]
        ga = a.grad.flatten()[q]
        if float(ga) == 0.0:
            continue
        seed = torch.zeros_like(z).flatten()
        seed[q] = ga
        g = torch.autograd.grad(z, leaves, grad_outputs=seed.view_as(z), retain_graph=True, allow_unused=True)
        for acc, gk in zip(bounds, g):
            if gk is not None:
                acc += gk.abs()
    return bounds


def relu_flip_allowance(params_np, nodes, edge_attr, edge_index, target, num_layers, m_steps, tau=1e-5, max_units=256, ln_eps=1e-5):
    """The gradient of a ReLU network is discontinuous where a pre-activation crosses zero: two evaluations that are both accurate to
    float32 rounding can disagree on the sign of a pre-activation that lies within rounding distance of zero, and then their
    gradients differ by what toggling that unit's ReLU derivative changes.  This returns, per parameter, an upper bound of that
    effect for THIS input (float64, first order): near_zero_units of the model's tape, flip_bounds of them on the parameters.
    Returns ({name: max |allowed change|}, number of such units)."""
    dtype = torch.float64
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in params_np.items()}
    tape = []
    out = epd_forward_taped(p, torch.tensor(nodes, dtype=dtype), torch.tensor(edge_attr, dtype=dtype),
                            torch.tensor(edge_index, dtype=torch.int64), num_layers, m_steps, tape, ln_eps)
    loss = F.l1_loss(out, torch.tensor(target, dtype=dtype), reduction="sum") / out.shape[0]
    loss.backward(retain_graph=True)
    units = near_zero_units(tape, tau, max_units)
    bounds = flip_bounds(tape, units, list(p.values()))
    return {k: float(v.max()) for k, v in zip(p, bounds)}, len(units)
