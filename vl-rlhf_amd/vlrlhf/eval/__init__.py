"""Benchmark evaluation on the HIP engine: the stage after SFT / DPO / generation in the reference's pipeline (src/vlrlhf/eval/**).

  python -m vlrlhf.eval.pope.eval       POPE (yes / no hallucination probes): acc, precision, recall, F1, yes-rate per question file
  python -m vlrlhf.eval.seedbench.eval  SEED-Bench image questions by perplexity; seedbench.calculate gives the accuracies
  python -m vlrlhf.eval.vqa.generate    free-form answers to a question file
  python -m vlrlhf.eval.mme.eval        MME prediction table for VLMEvalKit's scorer
  python -m vlrlhf.eval.merge_shards    joins the --num_shards outputs of any of them

Each takes a saved checkpoint or an adapter directory of any of the four model families (utils.load_model_and_processor)."""
