"""CPU: every entry of include/isr_hip.h that takes a non-const device output pointer is poisoned by a case of
tests/test_gpu_outputs_written.py (its ENTRIES table) or exempted below with a reason, so a new entry cannot skip that
suite unnoticed; and the table names tests that exist."""
import ast
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "isr_hip.h"
GPU_TESTS = Path(__file__).resolve().parent / "test_gpu_outputs_written.py"

# entry -> why test_gpu_outputs_written.py does not poison it
EXEMPT = {
    "isr_corr_argmax_recheck_count": "diagnostics: a HOST count read back from the workspace of the last call",
    "isr_corr_argmax_recheck_count_f32": "diagnostics: a HOST count read back from the workspace of the last call",
    "isr_corr_argmax_screen_redone": "diagnostics: HOST counts read back from the workspace of the last call",
    "isr_corr_argmax_clock_mhz": "diagnostics: a HOST clock read back from the workspace of the last call",
    "isr_epnp_host": "host-only: no device memory",
    "isr_epnp_jacobi_host": "host-only: no device memory",
    "isr_ransac_seq_host": "host-only: no device memory",
    "isr_bfgs_host_init": "host-only: no device memory",
    "isr_bfgs_host_step": "host-only: no device memory",
}
# parameters that are scratch or in-place state rather than outputs
NOT_OUTPUTS = {"ws", "state"}


def _declarations():
    """-> {entry: [(type, name)]} for every isr_* function declared in the header, whatever it returns.  Every `isr_name(`
    outside comments and #define lines must be one of them: a declaration this parser misreads fails here."""
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    out = {}
    for stmt in text.split(";"):
        stmt = re.split(r"[{}]", stmt)[-1]
        m = re.fullmatch(r"\s*([A-Za-z_][\w\s\*]*?)\b(isr_\w+)\s*\(([^()]*)\)\s*", stmt)
        if m:
            params = [p.strip() for p in m.group(3).split(",") if p.strip() and p.strip() != "void"]
            out[m.group(2)] = [tuple(re.match(r"(.*?)(\w+)$", p).groups()) for p in params]
    named = set(re.findall(r"\b(isr_\w+)\s*\(", text))
    assert named == set(out), f"declarations the parser did not read: {sorted(named - set(out))}"
    return out


def _device_outputs(params):
    return [name for typ, name in params if "*" in typ and not typ.strip().startswith("const") and name not in NOT_OUTPUTS]


def _gpu_table():
    tree = ast.parse(GPU_TESTS.read_text())
    table = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and any(getattr(t, "id", None) == "ENTRIES" for t in n.targets))
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    return table, tests


def test_header_parses():
    decls = _declarations()
    assert len(decls) > 60 and "isr_pnp_ransac_batch" in decls and "isr_rel_pose_table" in decls
    assert _device_outputs(decls["isr_select_top_batch"]) == ["keep", "M_dev", "thr_dev"]
    assert _device_outputs(decls["isr_tuning_set"]) == [] and _device_outputs(decls["isr_abi_version"]) == []


def test_every_output_writing_entry_is_poisoned_or_exempt():
    decls = _declarations()
    table, _ = _gpu_table()
    writers = {e for e, p in decls.items() if _device_outputs(p)}
    missing = sorted(writers - set(table) - set(EXEMPT))
    assert not missing, f"entries with device outputs that no poisoned case covers and no exemption names: {missing}"
    both = sorted(set(table) & set(EXEMPT))
    assert not both, f"entries both covered and exempted: {both}"


def test_table_names_real_entries_and_tests():
    decls = _declarations()
    table, tests = _gpu_table()
    assert not sorted(set(table) - set(decls)), "the table names entries the header does not declare"
    assert not sorted(set(EXEMPT) - set(decls)), "the exemptions name entries the header does not declare"
    for entry, names in table.items():
        assert names and all(n in tests for n in names), (entry, names)


def test_exemptions_have_no_device_outputs_or_say_why():
    decls = _declarations()
    for entry, why in EXEMPT.items():
        assert why.startswith(("host-only", "diagnostics")), entry
        if why.startswith("host-only"):
            assert entry.endswith(("_host", "_host_init", "_host_step")), entry
