"""SEED-Bench accuracies per question type and overall, from the answer file of seedbench.eval and the benchmark's question file (the
reference's src/vlrlhf/eval/seedbench/calculate.py without its MySQL reporter).

  python -m vlrlhf.eval.seedbench.calculate --result_file seedbench_result.json --anno_path SEED-Bench.json [--task image]"""
import argparse
import json

TASK_RANGES = dict(image=(1, 9), video=(10, 12))


def filter_questions(questions, task="all"):
    """task: "image" (types 1-9), "video" (10-12), "all", or one question_type_id as a string"""
    if task == "all":
        return questions
    if task in TASK_RANGES:
        lo, hi = TASK_RANGES[task]
        return [q for q in questions if lo <= q["question_type_id"] <= hi]
    try:
        wanted = int(task)
    except ValueError:
        raise ValueError(f"Invalid task: {task}") from None
    return [q for q in questions if q["question_type_id"] == wanted]


def accuracies(responses, questions, type_names):
    """responses {question_id: {"choice"}}, questions with answer / question_type_id, type_names {type id: name} ->
    {name without spaces: percent, ..., "Total": percent}, rounded to 2 places, types in the order their first question appears"""
    seen, right = {}, {}
    for q in questions:
        t = q["question_type_id"]
        seen[t] = seen.get(t, 0) + 1
        right[t] = right.get(t, 0) + (responses[q["question_id"]]["choice"] == q["answer"])
    out = {}
    for t, n in seen.items():
        out[type_names[t].replace(" ", "")] = round(right[t] / n * 100, 2)
        print(f"Data type {t}: {right[t] / n * 100:.2f}%")
    total = sum(right.values()) / sum(seen.values()) * 100
    print(f"Total accuracy: {total:.2f}%")
    out["Total"] = round(total, 2)
    return out


def calculate(result_file, anno_path, task="image"):
    with open(anno_path) as f:
        anno = json.load(f)
    type_names = {v: k for k, v in anno["question_type"].items()}
    with open(result_file) as f:
        responses = json.load(f)
    return accuracies(responses, filter_questions(anno["questions"], task), type_names)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--result_file", type=str, default="seedbench_result.json")
    p.add_argument("--anno_path", type=str, default="SEED-Bench.json")
    p.add_argument("--task", type=str, default="image")
    args = p.parse_args(argv)
    print(f"evaluating.. {args.result_file}")
    return calculate(args.result_file, args.anno_path, args.task)


if __name__ == "__main__":
    main()
