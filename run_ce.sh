#!/bin/bash
# Supervised cross-entropy baseline (reference main_ce.py recipe: 500 epochs, lr 0.2 at batch
# 256, scaled linearly to lr 0.8 at batch 1024, cosine), SyncBN, one process per GPU over RCCL.
# Fine-tuning a pretrained encoder on 10 % of the labels instead:
#   CKPT=path/to/last.pth ./run_ce.sh --label_frac 0.1 --learning_rate 0.05 --epochs 100
# Distilling a fine-tuned network into a student on all images (the SimCLRv2 stage 3):
#   ./run_ce.sh --distill_ckpt path/to/finetuned/last.pth --distill_model resnet50 --model resnet18
NGPU=${NGPU:-2}
export PYTHONPATH=.
python -m torch.distributed.run --nproc-per-node ${NGPU} --master-addr 127.0.0.1 --master-port 6016 main_ce.py \
    --syncBN \
    --batch_size 1024 \
    --learning_rate 0.8 \
    --cosine \
    --ngpu ${NGPU} ${CKPT:+--ckpt ${CKPT}} "$@"
