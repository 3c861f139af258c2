"""CPU: the layout and the refusals of Point-M2AE data-parallel pretraining (point_m2ae.ddp_segment, engine_pretrain_m2ae) --
every parameter in exactly one backward segment, each segment one contiguous range of the flat buffer in backward order, the
engine's checks, the look-ahead loader and run_epoch's visible-token overflow guard."""
from types import SimpleNamespace

import pytest
import torch


def _model():
    from gm3d_amd import point_m2ae as P
    torch.manual_seed(0)
    return P.PointM2AE()


def test_ddp_segment_assigns_every_parameter():
    from gm3d_amd import point_m2ae as P
    m = _model()
    segs = {n: P.ddp_segment(n) for n, _ in m.named_parameters()}
    assert set(segs.values()) == {0, 1, 2, 3}
    for n, s in segs.items():
        head = n.split(".")[0]
        if head in ("token_embed", "encoder_pos_embeds", "encoder_blocks"):
            assert s == 3 - int(n.split(".")[1]), n          # level 2 -> 1, level 1 -> 2, level 0 -> 3
        elif head == "encoder_norms":
            assert s == (3 if n.split(".")[1] == "0" else 0), n
        else:
            assert head in ("mask_token", "decoder_pos_embeds", "h_decoder", "token_prop", "decoder_norm", "rec_head",
                            "loss_pred_head") and s == 0, n


def test_each_segment_is_one_contiguous_range_in_backward_order():
    """FlatAdamWEma's layout rule (optim._split_decay): the decayed parameters segment by segment, ascending -- segment 0 (completed
    first by the backward) first; the non-decayed ones after the last segment, travelling with it."""
    from gm3d_amd import optim
    from gm3d_amd import point_m2ae as P
    m = _model()
    decay, no_decay = optim._split_decay(m, P.ddp_segment)
    order = [P.ddp_segment(n) for n, _ in decay]
    assert order == sorted(order) and sorted(set(order)) == [0, 1, 2, 3]
    assert len(decay) + len(no_decay) == len(list(m.parameters()))
    # every segment owns weights, and the block stacks keep their batched-weight-gradient grouping inside their segment
    for sg in range(4):
        names = [n for n, _ in decay if P.ddp_segment(n) == sg]
        assert names and any(".weight" in n for n in names)


def test_engine_refuses_unsupported_setups():
    from gm3d_amd import engine_pretrain_m2ae as EM
    from gm3d_amd import point_m2ae as P
    args = SimpleNamespace(accum_iter=1)
    plain = SimpleNamespace(segment_ranges=None)
    EM.check_setup(plain, args, 1)                                      # one GPU: any layout
    with pytest.raises(ValueError, match="segment"):
        EM.check_setup(plain, args, 2)
    pointmae_layout = SimpleNamespace(segment_ranges={0: (0, 8)})       # built with engine_pretrain.ddp_segment: one segment only
    with pytest.raises(ValueError, match="segment"):
        EM.check_setup(pointmae_layout, args, 2)
    EM.check_setup(SimpleNamespace(segment_ranges={k: (k, k + 1) for k in range(4)}), args, 2)
    with pytest.raises(NotImplementedError, match="accum_iter"):
        EM.check_setup(plain, SimpleNamespace(accum_iter=2), 1)
    with pytest.raises(NotImplementedError, match="accum_iter"):
        P.SegmentedM2AEStep(None, None, plain, SimpleNamespace(accum_iter=4), None, 0)


def test_look_ahead_loader_yields_in_order_with_the_next_batch():
    from gm3d_amd import streams
    batches = [torch.full((2, 4, 3), float(i)) for i in range(3)]
    la = streams.LookAhead(batches, lambda b: b.to(torch.device("cpu"), non_blocking=True))
    assert len(la) == 3
    seen = []
    for b in la:
        seen.append((float(b[0, 0, 0]), None if la.next is None else float(la.next[0, 0, 0])))
    assert seen == [(0.0, 1.0), (1.0, 2.0), (2.0, None)] and la.next is None


def test_run_epoch_raises_on_visible_token_overflow():
    """The flag is read where the finite-loss guard is read (every print_freq iterations)."""
    from gm3d_amd import engine_pretrain as E
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=0.1)
    args = SimpleNamespace(lr=0.1, min_lr=0.0, warmup_epochs=1, epochs=10, accum_iter=1)
    flag = torch.zeros(1, dtype=torch.int32)
    one = torch.ones(())

    def step(samples, it):
        if it == 2:
            flag.fill_(1)
        return {"loss": one, "loss_learn": one, "loss_mse": one * 0, "loss_chfr": one, "grad_norm": one, "vis_overflow": flag}

    loader = [torch.zeros(2, 4, 3) for _ in range(6)]
    with pytest.raises(RuntimeError, match="overflow.*iteration 3"):
        E.run_epoch(loader, opt, torch.device("cpu"), 0, args, step, None, print_freq=2, use_graph=False)
    flag.zero_()
    st = E.run_epoch(loader, opt, torch.device("cpu"), 0, args, lambda s, it: {k: v for k, v in step(s, -1).items()}, None,
                     print_freq=2, use_graph=False)
    assert st["loss"] == 2.0 and st["replayed_iters"] == 0
