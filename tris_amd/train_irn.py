"""Training IRNet's edge / displacement network on the MI355X, from the labels of the CRF pass to the weights make_ins_seg loads:
the reference's IRNet/step_refer/train_irn.py on this stack.

    python -m tris_amd.train_irn --train_list names.json --ir_label_out_dir L --voc12_root IMG --irn_backbone_weights R50.pth \\
        --irn_weights_name W.pth

  names.json   the JSON list of names (what validate_same_sentence(save_cam=True) writes as {dataset}_train_names.json)
  L/{name}.png the name's label, the image's size (what the reference's cam_to_ir_label writes)
  IMG/...      the image of the name: its id is name.split('_')[-1] (IRNet/voc12/dataloader.py:226-231)
  R50.pth      the ResNet-50 the reference downloads (IRNet/net/resnet50.py:6-8, :100-105), as a file: a state dict under that
               module's key names, or a full EdgeDisplacement state dict.  With a backbone-only file the heads keep torch's default
               initialisation under --seed, as the reference's constructors leave them.  This stack never downloads anything.
  W.pth        torch.save(trainer.state_dict()): what `python -m tris_amd.make_ins_seg --irn_weights_name` loads

The argument names are those of IRNet/run_sample_refer.py that train_irn.run reads; --num_workers is accepted and unused (the
batches come from the HBM cache: tris_amd.dataset.irn_data, where the random numbers are documented).
The labels come from `python -m tris_amd.cam_to_ir_label`.
Not here: data parallelism, graph capture of the step.
"""
import argparse
import time

BACKBONE_MESSAGE = ("--irn_backbone_weights FILE is required: the reference downloads its ResNet-50 (IRNet/net/resnet50.py:100-105), "
                    "this stack never downloads; give the file (a state dict under net/resnet50.py's key names, or a full "
                    "EdgeDisplacement state dict)")


def get_parser():
    p = argparse.ArgumentParser(description="IRNet edge / displacement training on the MI355X")
    p.add_argument("--train_list", required=True, help="JSON list of names")
    p.add_argument("--ir_label_out_dir", required=True, help="label directory ({name}.png)")
    p.add_argument("--voc12_root", required=True, help="image directory")
    p.add_argument("--irn_crop_size", default=512, type=int)
    p.add_argument("--irn_batch_size", default=32, type=int)
    p.add_argument("--irn_num_epoches", default=3, type=int)
    p.add_argument("--irn_learning_rate", default=0.1, type=float)
    p.add_argument("--irn_weight_decay", default=1e-4, type=float)
    p.add_argument("--irn_weights_name", required=True, help="where the trained state dict is saved")
    p.add_argument("--work_space", default=None)
    p.add_argument("--num_workers", default=0, type=int, help="accepted, unused")
    p.add_argument("--seed", default=0, type=int, help="order, augmentation and the heads' initialisation")
    p.add_argument("--irn_backbone_weights", default=None, help="ResNet-50 (or full EdgeDisplacement) state dict file")
    return p


def initial_network(weights_file, seed):
    """EdgeDisplacement with the file's tensors, on the CPU.  A file without head tensors is the backbone under net/resnet50.py's
    names: the heads keep torch's default initialisation under torch.manual_seed(seed)."""
    import torch
    from .irn_net import EdgeDisplacement
    torch.manual_seed(seed)
    net = EdgeDisplacement()
    sd = torch.load(weights_file, map_location="cpu")
    if not any(k.startswith("fc_edge") or ".fc_edge" in k for k in sd):
        own = net.state_dict()
        merged = {k: v for k, v in own.items() if not k.startswith("resnet50.")}
        trunk = {"resnet50." + k: v for k, v in sd.items() if "resnet50." + k in own}
        missing = [k for k in own if k.startswith("resnet50.") and k not in trunk]
        if missing:
            raise KeyError(f"{weights_file}: not a ResNet-50 state dict under net/resnet50.py's names: missing {len(missing)} "
                           f"tensors, first {missing[:3]}")
        merged.update(trunk)
        sd = merged
    net.load_state_dict(sd)
    return net


def run(args, log=print):
    if args.irn_backbone_weights is None:      # before any import that touches the GPU
        raise SystemExit(BACKBONE_MESSAGE)
    import torch
    from . import ops
    from .dataset.irn_data import HbmIrnCache, IrnLoader, ReferAffinityData
    from .irn_train import IrnTrainer
    if not torch.cuda.is_available():
        raise ops.NoGpuError("tris_amd.train_irn runs on MI355X only (no GPU in this process)")
    data = ReferAffinityData(args.train_list, args.ir_label_out_dir, args.voc12_root, args.irn_crop_size, rescale=(0.5, 1.5),
                             hor_flip=True, crop_method="random")
    B = args.irn_batch_size
    max_step = (len(data) // B) * args.irn_num_epoches
    if max_step == 0:
        raise ValueError(f"{len(data)} names make no batch of {B}")
    net = initial_network(args.irn_backbone_weights, args.seed).cuda()
    trainer = IrnTrainer(net, lr=args.irn_learning_rate, weight_decay=args.irn_weight_decay, max_step=max_step, radius=10)
    cache = HbmIrnCache(data, "cuda")
    log(f"{len(data)} names, {len(cache.image_offsets)} images, {cache.nbytes / 2 ** 20:.1f} MiB in HBM")
    loader = IrnLoader(cache, B, seed=args.seed, shuffle=True, drop_last=True)
    start = time.time()
    acc, n_acc = torch.zeros(4, device="cuda"), 0
    for ep in range(args.irn_num_epoches):
        log('Epoch %d/%d' % (ep + 1, args.irn_num_epoches))
        stage = time.time()
        for it, (img, _, label_reduced) in enumerate(loader):
            out = trainer.train_step(img, label_reduced)
            acc += out["losses"]                      # (on the device: the host reads the losses only where it prints them)
            n_acc += 1
            step = trainer.optimizer.global_step
            if (step - 1) % 50 == 0:
                mean = (acc / n_acc).tolist()
                acc.zero_()
                n_acc = 0
                eta = time.ctime(int(start + (time.time() - start) / (step / max_step)))
                log('step:%5d/%5d' % (step - 1, max_step), 'loss:%.4f %.4f %.4f %.4f' % tuple(mean),
                    'imps:%.1f' % ((it + 1) * B / (time.time() - stage)), 'lr: %.4f' % (trainer.optimizer.param_groups[0]['lr']),
                    'etc:%s' % eta, flush=True)
    log('Analyzing displacements mean ... ', end='')
    trainer.fit_mean_shift(IrnLoader.top_left(cache, B))
    log('done.')
    torch.save(trainer.state_dict(), args.irn_weights_name)
    return trainer


def main(argv=None):
    run(get_parser().parse_args(argv))


if __name__ == "__main__":
    main()
