"""TRIS Stage-2 training on MI355X -- drop-in for the reference's `train_stage2.py`: the pseudo-mask decoder trained with
`criterion` on the four heads (train_stage2.py:314-319), AdamW over the two parameter groups of `trainable_parameters`
(:133-138; as FusedAdamW), the poly-0.9 LambdaLR stepped once per EPOCH (:192 -- its lambda counts iterations, so the rate barely
decays; Stage-1 steps it per iteration), validation after every epoch with the best and best-hit checkpoints, `--resume --eval`,
and the final evaluation of the train split with the best checkpoint (:229-247).

    python -m tris_amd.train_stage2 --pseudo_path <dir> <the reference's flags>

Batches come from the HBM-resident loader (tris_amd.dataset.hbm; TRIS_HBM_LOADER=0: the reference's DataLoader): images,
targets and the pseudo masks -- each file summed and NEAREST-resized on the GPU once, when the cache is built -- are gathered on
the device per step.  The final evaluation of the train split reuses the training cache's images, so the split is decoded and
resized once per run.

Single GPU, eager steps (the reference's Stage-2 script is single-GPU: --distributed raises).  EMA consistency training
(--model_ema, :58-63, 302-312, 328-332) needs `ema_pytorch`, which is not on this stack: it raises, unless TRIS_STAGE2_EMA=1
(cfg.stage2_ema) selects this stack's restatement of that package (tris_amd.ema): the mean teacher runs forward
under no_grad on the same batch, four sigmoid-MSE terms join the loss as l5 (ops.seg_loss5) and the teacher is updated after every
optimiser step.  The aux ViT-B/32 the reference loads (:170) is never read by its train_one_epoch, with or without EMA, and is not
loaded.
"""
import datetime
import os
import time

import torch

from . import ops
from .config import cfg
from .train_stage1 import _logger, build_loader, setup_seed


def _check_args(args):
    if getattr(args, "model_ema", False):
        if not cfg.stage2_ema:
            raise NotImplementedError("--model_ema: EMA consistency training needs the ema_pytorch package (train_stage2.py:22), "
                                      "which is not on this stack; Stage-2 trains without EMA (l5 = 0).  TRIS_STAGE2_EMA=1 selects "
                                      "this stack's restatement of it (tris_amd.ema)")
        if getattr(args, "consistency_type", "mse") == "kl":
            raise ValueError("--consistency_type kl with --model_ema: the reference passes the teacher's raw logits to F.kl_div as "
                             "the target (train_stage2.py:286-288), so every negative logit gives NaN: there is nothing to reproduce")
    if getattr(args, "distributed", False):
        raise NotImplementedError("--distributed: the reference's Stage-2 script trains on a single GPU "
                                  "(scripts/train_stage2.sh); data-parallel Stage-2 is not implemented")


def train_step(model, optimizer, img, word_ids, pseudo, model_ema=None, consistency=False):
    """forward -> the four BCE losses -> backward -> AdamW, bracketed as one h2 step (train_stage1._step_body).
    -> device tensor losses[5] = (loss, l1, l2, l3, l4), detached (no host sync).
    model_ema (tris_amd.ema.EMA): its forward follows the student's under no_grad and it is updated behind the optimiser, all on
    the one stream (the reference's torch.cuda.synchronize(), :327, orders nothing here); consistency: the loss is ops.seg_loss5
    and -> losses[6] = (loss, l1, l2, l3, l4, l5)"""
    if consistency and model_ema is None:
        raise ValueError("consistency=True needs model_ema")
    ops.h2_begin_step()
    outs = model(img, word_ids)
    if model_ema is not None:
        with torch.no_grad():
            ema_outs = model_ema(img, word_ids)
    losses = ops.seg_loss5(outs, ema_outs, pseudo) if consistency else ops.bce4(outs, pseudo)
    optimizer.zero_grad()
    losses[0].backward()
    optimizer.step()
    if model_ema is not None:
        model_ema.update()
    ops.h2_end_step()
    return losses.detach()


def train_one_epoch(train_loader, model, optimizer, epoch, local_rank, args, iteration=0, clip_model=None, model_ema=None):
    """The reference's signature and batch-dict contract (train_stage2.py:260); returns `iteration`."""
    _check_args(args)
    if model_ema is not None and not cfg.stage2_ema:
        raise NotImplementedError("model_ema: EMA consistency training is off on this stack (TRIS_STAGE2_EMA=1 turns it on)")
    consistency = model_ema is not None and bool(getattr(args, "model_ema", False))     # (train_stage2.py:302)
    model.train()
    num_steps = len(train_loader)
    t0 = time.time()
    for idx, (samples, targets) in enumerate(train_loader):
        word_ids = samples["word_ids"].squeeze(1).cuda(local_rank, non_blocking=True)
        img = samples["img"].cuda(local_rank, non_blocking=True)
        pseudo = targets["pseudo_gt"].cuda(local_rank, non_blocking=True)
        last = train_step(model, optimizer, img, word_ids, pseudo, model_ema, consistency)
        if idx % args.print_freq == 0 and local_rank == 0:
            v = last.tolist() + [0.0]   # the only host sync, every print_freq steps (without EMA l5 is the reference's constant 0)
            print(f"Train:[{epoch:2d}/{args.epoch}][{idx:4d}/{num_steps}] | lr {optimizer.param_groups[0]['lr']:.6f} || "
                  f"loss: {v[0]:.4f} | l1: {v[1]:.4f} | l2: {v[2]:.4f} | l3: {v[3]:.4f} | l4: {v[4]:.4f} | l5: {v[5]:.4f} | "
                  f"time/step: {(time.time() - t0) / (idx + 1):.4f}", flush=True)
        iteration += 1
    print(f"EPOCH {epoch} training takes {datetime.timedelta(seconds=int(time.time() - t0))}", flush=True)
    return iteration


def build_dataset(args, split, train, eval_mode, pseudo_path=None, tokenizer=None):
    """ReferDataset with the reference's Stage-2 arguments (train_stage2.py:72-93)"""
    from .dataset.ReferDataset import ReferDataset
    from .dataset.transform import get_transform
    return ReferDataset(refer_data_root=args.refer_data_root, dataset=args.dataset, splitBy=args.splitBy,
                        bert_tokenizer=args.bert_tokenizer, split=split, size=args.size, max_tokens=args.max_query_len,
                        image_transforms=get_transform(args.size, train=train), eval_mode=eval_mode, pseudo_path=pseudo_path,
                        tokenizer=tokenizer)


def main(args, tokenizer=None):
    """tokenizer: as train_stage1.main (an extension; default the CLIP tokenizer)"""
    _check_args(args)
    from .model.model_stage2 import TRIS
    from .optim import FusedAdamW
    from .utils.util import load_checkpoint, load_pretrained_checkpoint, save_checkpoint
    from .validate import validate
    local_rank = 0
    log = _logger(args, local_rank)
    model = TRIS(args).cuda()
    model_ema = None
    if args.model_ema:
        # where the reference builds it (:58-63): before model.train() and before any checkpoint is loaded.  The copy keeps the modes
        # of this moment for good -- root and decoder in train mode, the CLIP backbone in eval mode (clip's build_model returns
        # .eval()) -- so the teacher's trunk runs on running statistics and its decoder BatchNorms on batch statistics
        from .ema import EMA
        model_ema = EMA(model)
    param_groups = model.trainable_parameters()
    model.train()
    log.info(f"number of params: {sum(p.numel() for p in model.parameters() if p.requires_grad) / 1e6:.2f}M")

    val_sets = [build_dataset(args, sp, train=False, eval_mode=True, tokenizer=tokenizer) for sp in args.test_split.split(",")]
    val_loaders = [build_loader(args, v, 1, False, False) for v in val_sets]

    def evaluate(loaders):
        return [validate(args, vl, model, local_rank, logger=log) for vl in loaders]

    optimizer = FusedAdamW([
        {"params": param_groups[0], "lr": args.lr * args.lr_multi, "weight_decay": args.weight_decay},
        {"params": param_groups[1], "lr": args.lr, "weight_decay": args.weight_decay},
    ], lr=args.lr, weight_decay=args.weight_decay)
    if model_ema is not None:
        model_ema.bind(optimizer)

    if args.resume and args.eval:
        load_checkpoint(args, model, optimizer, None, log)
        t0 = time.time()
        res = evaluate(val_loaders)
        acc = [float(r[1]) for r in res] + [0.0, 0.0]
        print(f"val: {acc[0]}, testA, {acc[1]}, testB: {acc[2]}")
        print(f"Testing time:  {datetime.timedelta(seconds=int(time.time() - t0))}")
        return res

    if args.pseudo_path is None:
        raise ValueError("Stage-2 training needs --pseudo_path (the directory of the pseudo masks)")
    train_set = build_dataset(args, "train", train=True, eval_mode=False, pseudo_path=args.pseudo_path,
                              tokenizer=tokenizer)
    train_loader = build_loader(args, train_set, args.batch_size, True, False)
    cache = getattr(train_loader, "cache", None)
    log.info(f"training batches from {type(train_loader).__name__}"
             + (f": {len(train_set)} refs, {cache.nbytes() / 2 ** 20:.1f} MiB resident, pseudo masks included" if cache is not None else ""))
    steps_total = max(len(train_loader) * args.epoch, 1)
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lambda x: (1 - x / steps_total) ** 0.9)
    if args.resume:
        load_checkpoint(args, model, optimizer, scheduler, log)
    if args.pretrained_checkpoint is not None:
        print("loading ", args.pretrained_checkpoint)
        load_pretrained_checkpoint(args.pretrained_checkpoint, model)

    log.info("Start training")
    best = {"val_acc": -1, "val_hit": -1, "epoch": -1, "path": "", "hit": -1, "hit_path": "", "testA": -1, "testB": -1}
    iteration, train_time, start = 0, 0.0, time.time()
    for epoch in range(args.start_epoch, args.epoch):
        t0 = time.time()
        iteration = train_one_epoch(train_loader, model, optimizer, epoch, local_rank, args, iteration, model_ema=model_ema)
        scheduler.step()                  # once per EPOCH, as train_stage2.py:192
        torch.cuda.synchronize()
        train_time += time.time() - t0
        res = evaluate(val_loaders)
        oIoU, val_acc, hit = res[0]
        if float(val_acc) > best["val_acc"]:
            if os.path.exists(best["path"]):
                os.remove(best["path"])
            best.update(path=save_checkpoint(epoch, model, optimizer, scheduler, log, args, f"ckpt_320_epoch_{epoch}.pth"),
                        val_acc=float(val_acc), val_hit=hit, epoch=epoch,
                        testA=float(res[1][1]) if len(res) > 1 else 0, testB=float(res[2][1]) if len(res) > 2 else 0)
        if hit > best["hit"]:
            if os.path.exists(best["hit_path"]):
                os.remove(best["hit_path"])
            best.update(hit_path=save_checkpoint(epoch, model, optimizer, scheduler, log, args, f"ckpt_320_epoch_{epoch}_hit.pth"),
                        hit=hit)
        print(best, flush=True)

    # the train split, evaluated with the best checkpoint (train_stage2.py:229-247)
    if best["path"]:
        print("loading ", best["path"])
        load_pretrained_checkpoint(best["path"], model)
        train_eval = build_loader(args, build_dataset(args, "train", train=False, eval_mode=True, tokenizer=tokenizer), 1, False,
                                  False, images_from=train_loader)
        oIoU, mIoU, hit = evaluate([train_eval])[0]
        print("Validat on the train split: ", oIoU, mIoU, hit)
    print(best)
    log.info(f"Training time {train_time:.1f}s; training + testing {datetime.timedelta(seconds=int(time.time() - start))}")
    return best


if __name__ == "__main__":
    from .args import get_parser
    _a = get_parser().parse_args()
    setup_seed(1234)
    main(_a)
