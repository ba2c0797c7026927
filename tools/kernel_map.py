"""Which launch of a cycle is which: for every operator of a resident hierarchy the kernels a V-cycle launches on it, keyed
the way rocprofv3's kernel trace shows them (kernel family + epilogue + grid size in workgroups), with the algorithmic bytes
of SURVEY.md 8(d) and the bytes the operator format that runs actually streams.  bench.py --kernel-map writes it next to
the trace; tools/summarize_prof.py joins it with the measured durations into the per-kernel roofline table.  Not product
code."""
import numpy as np



def _lanem_bytes(l_, n, vb):
    """bytes one merged sweep streams: the cluster layout (16-byte record per group, 4-byte unique codes, 8 + 2 bytes per slot, 12 bytes of row data)
    or the row / pair layout (12 bytes per slot, 32-byte record per row); plus b, x, hand-off buffer and snapshot"""
    if l_.get("cluster_rows"):
        return l_["units"] * 64 * (vb + 2) + l_["unique_units"] * 64 * 4 + l_["groups"] * 16 + n * (12 + 4 * vb)
    return l_["units"] * 64 * (vb + 4) + n * (32 + 4 * vb)


def _lanem_format(l_):
    if l_.get("cluster_rows"):
        return (f"clusters of <= {l_['cluster_rows']} rows per wave ({l_['rows'] / max(1, l_['groups']):.1f} on average), {l_['units'] / max(1, l_['groups']):.2f} x 64 slots and "
                f"{l_['unique_units'] / max(1, l_['groups']):.2f} x 64 unique operands per cluster, padded")
    return f"one row per wave, {l_['units'] / max(1, l_['rows']):.2f} x 64 operand slots per row, padded"

def _vec_bytes(epi, nr, nc, vb=8):
    return {"SET": vb * (nc + nr), "ACC": vb * (nc + 2 * nr), "RESID": vb * (nc + 2 * nr), "SUMSQ": vb * (nc + nr),
            "AXPBY": vb * (nc + 2 * nr), "ACC_AXPBY": vb * (nc + 3 * nr), "JACOBI": vb * (nc + 2 * nr), "JACOBI_B": vb * (nc + 2 * nr)}[epi]


def _op_entry(level, opname, dA, epi, what):
    inf = dA.info()
    nr, nc, nnz = inf["rows"], inf["cols"], inf["nnz"]
    vb = dA.dtype.itemsize
    vec = _vec_bytes(epi, nr, nc, vb)
    alg = (vb + 4) * nnz + 4 * (nr + 1) + vec
    npat, nval = dA.row_patterns(), dA.value_codes()
    masks = dA.row_masks() if npat else {"entries": 0}
    grid = int(inf["row_blocks"])
    if npat and masks["entries"]:
        streamed, form = nr + vec, ("row masks, lattice tiles 64 x 4 x %d (1 byte per row)" % masks["planes_per_lane"]) if (masks["lattice"] and epi != "SUMSQ") else "row masks (1 byte per row)"
        if epi != "SUMSQ":
            grid = int(masks["launch_grid"])
    elif npat:
        streamed, form = nr + vec, "row patterns (1 byte per row)"
    elif nval:
        streamed, form = 3 * nnz + 4 * (nr + 1) + vec, "16-bit columns + 8-bit value codes (3 bytes per entry)"
    else:
        streamed, form = (vb + 2) * nnz + 4 * (nr + 1) + vec, "16-bit columns + values as stored (10 bytes per entry)"
    return {"family": "csr", "epi": epi, "grid": grid, "level": level, "op": opname, "what": what,
            "rows": int(nr), "nnz": int(nnz), "bytes_alg": int(alg), "bytes_streamed": int(streamed), "format": form}


def kernel_map(dml, smoother_kind):
    nlev = len(dml.A)
    mats = list(dml._mats)
    out = []
    k = 0
    tail = dml.stats().get("dense_tail", {})
    t = tail["level"] if tail.get("built") and tail.get("applications") else nlev
    for i in range(nlev):
        if i == t:
            # the tail of the hierarchy as one dense operator (csrc/pamg_solver.hip, DenseTail): every launch of the levels >= t is replaced by
            # x_t = M b_t -- M streamed once, b_t read, x_t written
            n, vb = tail["rows"], dml.dtype.itemsize
            out.append({"family": "dense_tail", "grid": (n + 3) // 4, "level": i, "op": "M", "what": "tail of the hierarchy as one dense operator",
                        "rows": int(n), "nnz": int(n * n), "bytes_alg": int(vb * n * n + 2 * vb * n), "bytes_streamed": int(vb * n * n + 2 * vb * n),
                        "format": f"dense {n} x {n}, row-major, one wave per row"})
            break
        A = mats[k]; k += 1
        P = R = None
        if i < nlev - 1:
            P, R = mats[k], mats[k + 1]
            k += 2
        if i == 0:
            out.append(_op_entry(i, "A", A, "SUMSQ", "convergence-check norm ||b - A x||"))
        if i < nlev - 1:
            out.append(_op_entry(i, "A", A, "RESID", "residual r = b - A x"))
            out.append(_op_entry(i, "R", R, "SET", "restriction b_c = R r"))
            out.append(_op_entry(i, "P", P, "ACC", "prolongation x += P x_c"))
            inf = A.info()
            n, nnz, vb = inf["rows"], inf["nnz"], A.dtype.itemsize
            if smoother_kind == "gauss_seidel":
                alg = (vb + 4) * nnz + 4 * (n + 1) + 3 * vb * n
                sym = A.sym_info()
                directions = ((0, "forward"), (1, "backward"))
                dt = A.dense_tri_info()
                if dt["built"] and (dt["zero_launches"] or dt["correction_launches"]):
                    # the dense block-triangular form (csrc/pamg_dtri.hip): both sweeps of the level are 4 blocks - 2 plain launches each, a sparse and a
                    # dense phase per block step and direction.  One entry per (phase, direction, grid): bytes of ONE launch -- a block's inverse triangle
                    # resp. its share of the off-block slices, and the vectors; the ragged last block has grids of its own.  A launch IS one step of the
                    # dependency chain, so a row's dependency_levels is 1 (us per dependency level = the launch's time); the chain of one sweep is `block_steps`
                    directions = ()
                    B, nb = dt["block_rows"], dt["blocks"]
                    sizes = sorted({min(B, n - k * B) for k in range(nb)}, reverse=True)
                    steps = f"{2 * nb} block steps of <= {B} rows per sweep, {dt['kernel_launches']} launches"
                    if dt["correction_launches"]:
                        r_ = _op_entry(i, "A", A, "RESID", "A residual for the post-smoothing correction")
                        r_["shares_launches_with"] = "residual r = b - A x"
                        out.append(r_)
                    for m in sizes:
                        tri = vb * sum((r + 2) & ~1 for r in range(m))
                        for dirn in ("forward", "backward"):
                            out.append({"family": "gs_dtri_dense", "grid": (m + 1) // 2, "level": i, "op": "A",
                                        "what": f"dense phase, {dirn}: y_k = W_k t_k ({steps})", "rows": int(m), "nnz": int(nnz), "bytes_alg": int(tri + 3 * vb * m),
                                        "bytes_streamed": int(tri + 4 * vb * m), "format": f"packed inverse triangle of {m} rows, rows padded to 16 bytes", "dependency_levels": 1, "block_steps": int(2 * nb)})
                            out.append({"family": "gs_dtri_sparse", "grid": (16 * m + 255) // 256, "level": i, "op": "A",
                                        "what": f"sparse phase, {dirn}: t_k = rhs_k - off-block slice . v ({steps})", "rows": int(m), "nnz": int(dt["off_block_entries"] // 2),
                                        "bytes_alg": int((vb + 4) * dt["off_block_entries"] // 2 * m // n + 3 * vb * m),
                                        "bytes_streamed": int((vb + 4) * dt["off_block_entries"] // 2 * m // n + (2 * vb + 8) * m + 64 * dt["off_block_entries"] // 2 * m // n),
                                        "format": "CSR slice of the off-block entries, 16 lanes per row", "dependency_levels": 1, "block_steps": int(2 * nb)})
                elif sym["launches"] and sym["form"] != "none":
                    # the fused symmetric sweep: ONE launch walks both schedules (bytes: the two directions' together)
                    directions = ()
                    lm, ln = [A.lanem_info(w) for w in (0, 1)], [A.line_info(w) for w in (0, 1)]
                    if sym["form"] == "line":
                        out.append({"family": "gs_line", "grid": int(sym["launch_grid"]), "level": i, "op": "A",
                                    "what": f"symmetric Gauss-Seidel sweep, one launch (fast order, line scan: {ln[0]['lines']} lines, {ln[0]['line_levels']} + {ln[1]['line_levels']} line levels)",
                                    "rows": int(n), "nnz": int(nnz), "bytes_alg": int(2 * alg),
                                    "bytes_streamed": int(sum(l_["chunks"] * 64 * (l_["slots_per_row"] * (vb + 4) + 2 * vb + 1) + n * 4 * vb for l_ in ln)),
                                    "format": f"chunks of 64 rows x {ln[0]['slots_per_row']} slots", "dependency_levels": int(ln[0]["line_levels"] + ln[1]["line_levels"])})
                    else:
                        out.append({"family": "gs_lanem", "grid": int(sym["launch_grid"]), "level": i, "op": "A",
                                    "what": f"symmetric Gauss-Seidel sweep, one launch (fast order, merged: {lm[0]['super_levels']} + {lm[1]['super_levels']} super-levels of <= {lm[0]['s_max']} dependency levels)",
                                    "rows": int(n), "nnz": int(nnz), "bytes_alg": int(2 * alg),
                                    "bytes_streamed": int(sum(_lanem_bytes(l_, n, vb) for l_ in lm)),
                                    "format": _lanem_format(lm[0]),
                                    "dependency_levels": int(lm[0]["super_levels"] + lm[1]["super_levels"])})
                        if sym.get("zero_plan_launches"):
                            # the pre-smoothing launch of a level the cycle enters with x = 0: the zero-iterate plans (tune key 39) in the kernel's
                            # `zero` instantiation -- the forward plan of tril(A), the backward plan of triu(A), and the numerator vector (written, read)
                            zm = [A.lanem_info(w) for w in (4, 5)]
                            out.append({"family": "gs_lanem_zero", "grid": int(zm[0]["launch_grid"]), "level": i, "op": "A",
                                        "what": f"symmetric GS sweep from x = 0, one launch (zero-iterate plans: {zm[0]['super_levels']} + {zm[1]['super_levels']} super-levels of <= {zm[0]['s_max']} dependency levels)",
                                        "rows": int(n), "nnz": int(nnz), "bytes_alg": int(2 * alg),
                                        "bytes_streamed": int(sum(_lanem_bytes(l_, n, vb) for l_ in zm) + 2 * vb * n),
                                        "format": _lanem_format(zm[0]),
                                        "dependency_levels": int(zm[0]["super_levels"] + zm[1]["super_levels"])})
                        if sym.get("correction_launches"):
                            # the steps from x != 0 in correction form (tune key 41): the whole-operator residual kernel once more (the same kernel and grid
                            # as the residual in front of the restriction: the trace cannot tell the two apart, summarize_prof.py shares the launches out),
                            # then the zero-iterate plans in the kernel's accumulating instantiation (x is read and written once more than in `zero`)
                            r_ = _op_entry(i, "A", A, "RESID", "A residual for the post-smoothing correction")
                            r_["shares_launches_with"] = "residual r = b - A x"
                            out.append(r_)
                            out.append({"family": "gs_lanem_corr", "grid": int(zm[0]["launch_grid"]), "level": i, "op": "A",
                                        "what": f"correction sweep x += sweep(0, r), one launch (zero-iterate plans: {zm[0]['super_levels']} + {zm[1]['super_levels']} super-levels)",
                                        "rows": int(n), "nnz": int(nnz), "bytes_alg": int(2 * alg),
                                        "bytes_streamed": int(sum(_lanem_bytes(l_, n, vb) for l_ in zm) + 3 * vb * n),
                                        "format": _lanem_format(zm[0]),
                                        "dependency_levels": int(zm[0]["super_levels"] + zm[1]["super_levels"])})
                for which, dirn in directions:
                    lane, tile, line, lanem = A.lane_info(which), A.tile_info(which), A.line_info(which), A.lanem_info(which)
                    if lanem["rows"] and lanem["launch_grid"]:
                        out.append({"family": "gs_lanem", "grid": int(lanem["launch_grid"]), "level": i, "op": "A",
                                    "what": f"{dirn} Gauss-Seidel sweep (fast order, merged: {lanem['super_levels']} super-levels of <= {lanem['s_max']} dependency levels)",
                                    "rows": int(n), "nnz": int(nnz), "bytes_alg": int(alg), "bytes_streamed": int(_lanem_bytes(lanem, n, vb)),
                                    "format": _lanem_format(lanem), "dependency_levels": int(lanem["super_levels"])})
                    elif line["lines"] and line["launch_grid"]:
                        out.append({"family": "gs_line", "grid": int(line["launch_grid"]), "level": i, "op": "A", "what": f"{dirn} Gauss-Seidel sweep (fast order, line scan: {line['lines']} lines, {line['line_levels']} line levels)",
                                    "rows": int(n), "nnz": int(nnz), "bytes_alg": int(alg), "bytes_streamed": int(line["chunks"] * 64 * (line["slots_per_row"] * (vb + 4) + 2 * vb + 1) + n * 4 * vb),
                                    "format": f"chunks of 64 rows x {line['slots_per_row']} slots", "dependency_levels": int(line["line_levels"])})
                    elif lane["groups"] and lane["launch_grid"]:
                        out.append({"family": "gs_lane", "grid": int(lane["launch_grid"]), "level": i, "op": "A", "what": f"{dirn} Gauss-Seidel sweep (fast order, {lane['lanes_per_row']} lanes per row)",
                                    "rows": int(n), "nnz": int(nnz), "bytes_alg": int(alg), "bytes_streamed": int(lane["entry_slots"] * (vb + 4) + n * (4 + 4 * vb)),
                                    "format": f"{lane['lanes_per_row']} lanes x {lane['slots_per_lane']} slots per row, padded", "dependency_levels": int(inf["gs_levels_fwd"])})
                    elif tile["tiles"]:
                        out.append({"family": "gs_tile", "grid": int(tile["tiles"]), "level": i, "op": "A", "what": f"{dirn} Gauss-Seidel sweep (order-exact, tiled)",
                                    "rows": int(n), "nnz": int(nnz), "bytes_alg": int(alg), "bytes_streamed": None, "format": "step blocks", "dependency_levels": int(inf["gs_levels_fwd"])})
                    else:
                        out.append({"family": "gs_gran", "grid": None, "level": i, "op": "A", "what": f"{dirn} Gauss-Seidel sweep (order-exact)",
                                    "rows": int(n), "nnz": int(nnz), "bytes_alg": int(alg), "bytes_streamed": None, "format": "level-permuted CSR", "dependency_levels": int(inf["gs_levels_fwd"])})
            elif smoother_kind in ("block_gauss_seidel", "block_jacobi") or (A.op.fmt == "bsr" and A.op.blocksize[0] > 1 and smoother_kind in ("gauss_seidel", "jacobi")):
                # square-block levels: SURVEY 8(d) BSR(R x C) bytes = 8 R C nblk + 4 nblk + 4 (n_brow + 1) + vectors (x read, b read, x
                # written) + the inverted diagonal blocks of the block smoothers (8 R^2 per block row)
                bs = int(A.op.blocksize[0])
                nbrow = n // bs
                nblk = nnz // (bs * bs)
                block = smoother_kind.startswith("block_")
                alg = vb * bs * bs * nblk + 4 * nblk + 4 * (nbrow + 1) + 3 * vb * n + (vb * bs * bs * nbrow if block else 0)
                gs = smoother_kind.endswith("gauss_seidel")
                kind = ("BLK_GS" if block else "PNT_GS") if gs else ("BLK_JACOBI" if block else "PNT_JACOBI")
                blanes = [A.lane_info(w) for w in (0, 1)] if (gs and block) else []
                if gs and block and any(l_["groups"] and l_["launch_grid"] for l_ in blanes):
                    # fast order (csrc/pamg_blane.hip): one entry per direction; streamed = the padded block slots (values + block column), the
                    # block row of every slot row, b / Dinv / the result, the hand-off buffer (filled, written, polled) and x
                    for which, dirn in ((0, "forward"), (1, "backward")):
                        l_ = blanes[which]
                        if not (l_["groups"] and l_["launch_grid"]):
                            continue
                        rpw = 64 // l_["lanes_per_row"]
                        out.append({"family": "bsr_lane", "kind": kind, "bs": bs, "grid": int(l_["launch_grid"]), "level": i, "op": "A",
                                    "what": f"{dirn} block Gauss-Seidel sweep on BSR({bs},{bs}) (fast order, {l_['lanes_per_row']} lanes per block row)",
                                    "rows": int(n), "nnz": int(nnz), "bytes_alg": int(alg),
                                    "bytes_streamed": int(l_["entry_slots"] * (vb * bs * bs + 4) + l_["groups"] * rpw * 4 + n * 5 * vb + vb * bs * bs * nbrow),
                                    "format": f"{l_['lanes_per_row']} lanes x {l_['slots_per_lane']} blocks per block row, padded", "dependency_levels": int(inf["gs_levels_fwd"])})
                elif gs:
                    out.append({"family": "bsr_gs", "kind": kind, "bs": bs, "grid": None, "level": i, "op": "A",
                                "what": f"{'block' if block else 'point'} Gauss-Seidel sweep on BSR({bs},{bs}) (order-exact; forward and backward launches)",
                                "rows": int(n), "nnz": int(nnz), "bytes_alg": int(alg), "bytes_streamed": int(alg + 4 * nbrow), "format": f"level-permuted BSR({bs},{bs}) + row ids",
                                "dependency_levels": int(inf["gs_levels_fwd"])})
                else:
                    out.append({"family": "bsr_stream", "kind": kind, "bs": bs, "grid": int(inf["row_blocks"]), "level": i, "op": "A",
                                "what": f"{'block' if block else 'point'} Jacobi sweep on BSR({bs},{bs})", "rows": int(n), "nnz": int(nnz), "bytes_alg": int(alg),
                                "bytes_streamed": int(alg), "format": f"BSR({bs},{bs}) as stored"})
            elif smoother_kind == "jacobi":
                out.append(_op_entry(i, "A", A, "JACOBI", "weighted Jacobi sweep"))
                out.append(_op_entry(i, "A", A, "JACOBI_B", "weighted Jacobi sweep (BSR(1,1) levels)"))
            elif smoother_kind == "chebyshev":
                out.append(_op_entry(i, "A", A, "AXPBY", "Horner step h = c r + A h"))
                out.append(_op_entry(i, "A", A, "ACC_AXPBY", "last Horner step folded with x += h"))
                out.append(_op_entry(i, "A", A, "SET", "first product of the polynomial (x = 0)"))
    return out
