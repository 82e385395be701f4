//! `Evaluator::evaluate_h` (halo2_proofs/src/plonk/evaluation.rs:280-522) through the engine: the `#[repr(C)]` mirrors of
//! include/halo2hip.h's structures, and an owning builder (`FlatGraph`) that halo2_proofs fills from its private
//! `GraphEvaluator` (patches/0003-evaluate-h.patch adds the two `flat()` methods that do so).
use std::os::raw::c_int;

// ---- include/halo2hip.h: enums ------------------------------------------------------------------------------------
pub const H2HIP_VS_CONSTANT: u32 = 0;
pub const H2HIP_VS_INTERMEDIATE: u32 = 1;
pub const H2HIP_VS_FIXED: u32 = 2;
pub const H2HIP_VS_ADVICE: u32 = 3;
pub const H2HIP_VS_INSTANCE: u32 = 4;
pub const H2HIP_VS_CHALLENGE: u32 = 5;
pub const H2HIP_VS_BETA: u32 = 6;
pub const H2HIP_VS_GAMMA: u32 = 7;
pub const H2HIP_VS_THETA: u32 = 8;
pub const H2HIP_VS_Y: u32 = 9;
pub const H2HIP_VS_PREVIOUS: u32 = 10;

pub const H2HIP_CALC_ADD: u32 = 0;
pub const H2HIP_CALC_SUB: u32 = 1;
pub const H2HIP_CALC_MUL: u32 = 2;
pub const H2HIP_CALC_SQUARE: u32 = 3;
pub const H2HIP_CALC_DOUBLE: u32 = 4;
pub const H2HIP_CALC_NEGATE: u32 = 5;
pub const H2HIP_CALC_HORNER: u32 = 6;
pub const H2HIP_CALC_STORE: u32 = 7;

pub const H2HIP_ANY_ADVICE: u32 = 0;
pub const H2HIP_ANY_FIXED: u32 = 1;
pub const H2HIP_ANY_INSTANCE: u32 = 2;

// ---- include/halo2hip.h: structures (field for field, same order) ----------------------------------------------------
/// `ValueSource` (evaluation.rs:37-60): `kind` = H2HIP_VS_*, `a` = constant / intermediate / challenge / column index,
/// `b` = index into the graph's rotations for Fixed / Advice / Instance.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct h2hip_value_source {
    pub kind: u32,
    pub a: u32,
    pub b: u32,
}

/// `Calculation` + `CalculationInfo` (evaluation.rs:108-127, :213-219).  Horner: `x` = start value, `y` = factor, the
/// parts are `h2hip_graph::parts[parts_offset .. parts_offset + parts_count]`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct h2hip_calculation {
    pub op: u32,
    pub target: u32,
    pub x: h2hip_value_source,
    pub y: h2hip_value_source,
    pub parts_offset: u32,
    pub parts_count: u32,
}

/// `GraphEvaluator` (evaluation.rs:191-201); borrowed view of a `FlatGraph`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct h2hip_graph {
    pub constants: *const u64, // n_constants x 4 limbs, Montgomery form
    pub n_constants: u32,
    pub rotations: *const i32,
    pub n_rotations: u32,
    pub calculations: *const h2hip_calculation,
    pub n_calculations: u32,
    pub parts: *const h2hip_value_source,
    pub n_parts: u32,
    pub num_intermediates: u32,
}

/// Everything one circuit instance of `evaluate_h` reads.  Pointers are host pointers for `h2hip_evaluate_h_bn254`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct h2hip_evalh_desc {
    pub k: u32,
    pub extended_k: u32,
    pub extended_omega: *const u64,
    pub g_coset: *const u64,
    pub g_coset_inv: *const u64,
    pub n_fixed: u32,
    pub n_advice: u32,
    pub n_instance: u32,
    pub n_challenges: u32,
    pub fixed_cosets: *const *const u64,
    pub advice_polys: *const *const u64,
    pub instance_polys: *const *const u64,
    pub challenges: *const u64,
    pub y: *const u64,
    pub beta: *const u64,
    pub gamma: *const u64,
    pub theta: *const u64,
    pub l0: *const u64,
    pub l_last: *const u64,
    pub l_active_row: *const u64,
    pub custom_gates: h2hip_graph,
    pub n_perm_sets: u32,
    pub n_perm_columns: u32,
    pub chunk_len: u32,
    pub last_rotation: i32,
    pub perm_product_cosets: *const *const u64,
    pub perm_column_kind: *const u32,
    pub perm_column_index: *const u32,
    pub perm_cosets: *const *const u64,
    pub zeta: *const u64,
    pub delta: *const u64,
    pub n_lookups: u32,
    pub lookup_graphs: *const h2hip_graph,
    pub lookup_product_polys: *const *const u64,
    pub lookup_permuted_input_polys: *const *const u64,
    pub lookup_permuted_table_polys: *const *const u64,
}

/// `h2hip_evalh_parts_desc`: `h2hip_evalh_desc` with every column a coefficient-form polynomial of 2^k elements -- the proving key's
/// too -- followed by the range of parts (cosets of the 2^k domain) a call computes and the optional `t_evaluations`.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct EvalhPartsDesc {
    pub k: u32,
    pub extended_k: u32,
    pub extended_omega: *const u64,
    pub g_coset: *const u64,
    pub g_coset_inv: *const u64,
    pub n_fixed: u32,
    pub n_advice: u32,
    pub n_instance: u32,
    pub n_challenges: u32,
    pub fixed_polys: *const *const u64,
    pub advice_polys: *const *const u64,
    pub instance_polys: *const *const u64,
    pub challenges: *const u64,
    pub y: *const u64,
    pub beta: *const u64,
    pub gamma: *const u64,
    pub theta: *const u64,
    pub l0_poly: *const u64,
    pub l_last_poly: *const u64,
    pub l_active_row_poly: *const u64,
    pub custom_gates: h2hip_graph,
    pub n_perm_sets: u32,
    pub n_perm_columns: u32,
    pub chunk_len: u32,
    pub last_rotation: i32,
    pub perm_product_polys: *const *const u64,
    pub perm_column_kind: *const u32,
    pub perm_column_index: *const u32,
    pub perm_polys: *const *const u64,
    pub zeta: *const u64,
    pub delta: *const u64,
    pub n_lookups: u32,
    pub lookup_graphs: *const h2hip_graph,
    pub lookup_product_polys: *const *const u64,
    pub lookup_permuted_input_polys: *const *const u64,
    pub lookup_permuted_table_polys: *const *const u64,
    pub part_begin: u32,
    pub part_count: u32,
    pub t_evaluations: *const u64,
}

/// `h2hip_evalh_shuffles`: the shuffle arguments of one circuit instance, beside either description.  `graphs` holds two graphs per
/// shuffle (input side, shuffle side), `product_polys` one coefficient-form polynomial of 2^k elements per shuffle.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct EvalhShuffles {
    pub n_shuffles: u32,
    pub graphs: *const h2hip_graph,
    pub product_polys: *const *const u64,
}

/// `h2hip_evalh_mvlookups`: the logUp (mv-lookup) arguments of one circuit instance, beside either description.  Argument j has
/// `n_inputs[j]` input tuples sharing one table; `graphs` holds its input graphs, then its table graph, behind those of argument j - 1;
/// `phi_polys` / `m_polys` hold one coefficient-form polynomial of 2^k elements per argument (the grand sum, the multiplicities).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct EvalhMvLookups {
    pub n_args: u32,
    pub n_inputs: *const u32,
    pub graphs: *const h2hip_graph,
    pub phi_polys: *const *const u64,
    pub m_polys: *const *const u64,
}

// ---- owning builder -------------------------------------------------------------------------------------------------
/// A `GraphEvaluator` flattened into plain vectors.  halo2_proofs builds one per graph once per proving key; `view()`
/// lends it to the engine for the duration of a call.
#[derive(Clone, Debug, Default)]
pub struct FlatGraph {
    pub constants: Vec<[u64; 4]>,
    pub rotations: Vec<i32>,
    pub calculations: Vec<h2hip_calculation>,
    pub parts: Vec<h2hip_value_source>,
    pub num_intermediates: u32,
}

impl FlatGraph {
    pub fn vs(kind: u32, a: usize, b: usize) -> h2hip_value_source {
        h2hip_value_source { kind, a: a as u32, b: b as u32 }
    }

    /// a calculation with at most two operands (everything but Horner)
    pub fn push(&mut self, op: u32, target: usize, x: h2hip_value_source, y: h2hip_value_source) {
        self.calculations.push(h2hip_calculation { op, target: target as u32, x, y, parts_offset: 0, parts_count: 0 });
    }

    /// `Calculation::Horner(start, parts, factor)` (evaluation.rs:122-123)
    pub fn push_horner(&mut self, target: usize, start: h2hip_value_source, parts: &[h2hip_value_source], factor: h2hip_value_source) {
        let parts_offset = self.parts.len() as u32;
        self.parts.extend_from_slice(parts);
        self.calculations.push(h2hip_calculation {
            op: H2HIP_CALC_HORNER,
            target: target as u32,
            x: start,
            y: factor,
            parts_offset,
            parts_count: parts.len() as u32,
        });
    }

    /// borrowed C view; valid while `self` is neither moved nor modified
    pub fn view(&self) -> h2hip_graph {
        h2hip_graph {
            constants: self.constants.as_ptr() as *const u64,
            n_constants: self.constants.len() as u32,
            rotations: self.rotations.as_ptr(),
            n_rotations: self.rotations.len() as u32,
            calculations: self.calculations.as_ptr(),
            n_calculations: self.calculations.len() as u32,
            parts: self.parts.as_ptr(),
            n_parts: self.parts.len() as u32,
            num_intermediates: self.num_intermediates,
        }
    }
}

impl FlatGraph {
    /// append a constant (`GraphEvaluator::constants`); false when `F` is not bn256::Fr
    pub fn push_constant<F: 'static>(&mut self, c: &F) -> bool {
        match limbs_of(c) {
            Some(l) => {
                self.constants.push(l);
                true
            }
            None => false,
        }
    }
}

/// the 4 Montgomery limbs of a bn256::Fr (None for any other type)
pub fn limbs_of<F: 'static>(x: &F) -> Option<[u64; 4]> {
    if std::any::TypeId::of::<F>() != std::any::TypeId::of::<halo2curves::bn256::Fr>() || std::mem::size_of::<F>() != 32 {
        return None;
    }
    Some(unsafe { std::mem::transmute_copy::<F, [u64; 4]>(x) })
}

/// One circuit instance of `evaluate_h` described with borrowed slices: what halo2_proofs (which forbids unsafe code) hands
/// over.  Column slices are the `Polynomial`s' value vectors (`Deref<Target = [F]>`, poly.rs:116-128).
pub struct EvalHInput<'a, F> {
    pub k: u32,
    pub extended_k: u32,
    pub extended_omega: F,
    pub g_coset: F,
    pub g_coset_inv: F,
    /// pk.fixed_cosets (2^extended_k each)
    pub fixed_cosets: Vec<&'a [F]>,
    /// advice / instance polynomials in coefficient form (2^k each); the engine forms their cosets (evaluation.rs:306-323)
    pub advice_polys: Vec<&'a [F]>,
    pub instance_polys: Vec<&'a [F]>,
    pub challenges: &'a [F],
    pub y: F,
    pub beta: F,
    pub gamma: F,
    pub theta: F,
    /// pk.l0 / l_last / l_active_row (2^extended_k each)
    pub l0: &'a [F],
    pub l_last: &'a [F],
    pub l_active_row: &'a [F],
    pub custom_gates: &'a FlatGraph,
    /// sets[i].permutation_product_coset (2^extended_k each); empty skips the permutation argument
    pub perm_product_cosets: Vec<&'a [F]>,
    /// (H2HIP_ANY_*, column index) of cs.permutation.columns[j]
    pub perm_columns: Vec<(u32, u32)>,
    /// pk.permutation.cosets[j] (2^extended_k each)
    pub perm_cosets: Vec<&'a [F]>,
    /// cs.degree() - 2
    pub chunk_len: u32,
    /// -(cs.blinding_factors() + 1)
    pub last_rotation: i32,
    pub zeta: F,
    pub delta: F,
    pub lookup_graphs: &'a [FlatGraph],
    /// lookup.product_poly / permuted_input_poly / permuted_table_poly, coefficient form (2^k each)
    pub lookup_product_polys: Vec<&'a [F]>,
    pub lookup_permuted_input_polys: Vec<&'a [F]>,
    pub lookup_permuted_table_polys: Vec<&'a [F]>,
}

/// The shuffle arguments of one circuit instance (the argument of upstream PSE halo2: include/halo2hip.h, `h2hip_evalh_shuffles`):
/// `graphs[2 j]` and `graphs[2 j + 1]` are the input and the shuffle side of shuffle j, `product_polys[j]` its grand product in
/// coefficient form (2^k elements).
pub struct ShufflesInput<'a, F> {
    pub graphs: &'a [FlatGraph],
    pub product_polys: Vec<&'a [F]>,
}

/// the C view of a `ShufflesInput` and the tables it points into; None when the lengths do not fit
fn shuffles_view<F>(sh: &ShufflesInput<'_, F>, n: usize) -> Option<(Vec<h2hip_graph>, Vec<*const u64>)> {
    if sh.graphs.len() != 2 * sh.product_polys.len() || !sh.product_polys.iter().all(|s| s.len() == n) {
        return None;
    }
    Some((sh.graphs.iter().map(|g| g.view()).collect(), sh.product_polys.iter().map(|s| s.as_ptr() as *const u64).collect()))
}

/// The mv-lookup arguments of one circuit instance (include/halo2hip.h, `h2hip_evalh_mvlookups`): `n_inputs[j]` input graphs and one
/// table graph per argument, consecutively in `graphs`; `phi_polys[j]` / `m_polys[j]` its grand sum and multiplicities in coefficient
/// form (2^k elements).
pub struct MvLookupsInput<'a, F> {
    pub n_inputs: &'a [u32],
    pub graphs: &'a [FlatGraph],
    pub phi_polys: Vec<&'a [F]>,
    pub m_polys: Vec<&'a [F]>,
}

/// the C view of an `MvLookupsInput` and the tables it points into; None when the lengths do not fit
#[allow(clippy::type_complexity)]
fn mvlookups_view<F>(mv: &MvLookupsInput<'_, F>, n: usize) -> Option<(Vec<h2hip_graph>, Vec<*const u64>, Vec<*const u64>)> {
    let n_graphs: usize = mv.n_inputs.iter().map(|&k| k as usize + 1).sum();
    if mv.graphs.len() != n_graphs || mv.phi_polys.len() != mv.n_inputs.len() || mv.m_polys.len() != mv.n_inputs.len() {
        return None;
    }
    if mv.n_inputs.iter().any(|&k| !(1..=255).contains(&k)) || !mv.phi_polys.iter().chain(mv.m_polys.iter()).all(|s| s.len() == n) {
        return None;
    }
    let ptrs = |cols: &[&[F]]| -> Vec<*const u64> { cols.iter().map(|c| c.as_ptr() as *const u64).collect() };
    Some((mv.graphs.iter().map(|g| g.view()).collect(), ptrs(&mv.phi_polys), ptrs(&mv.m_polys)))
}

/// Safe front of `h2hip_evaluate_h_bn254`: checks the element type and every slice length, builds the pointer tables, calls
/// the engine.  `values` (2^extended_k elements) is read and written.  false: the engine declined, run the CPU body.
pub fn try_evaluate_h<F: 'static + Copy>(inp: &EvalHInput<'_, F>, values: &mut [F]) -> bool {
    evaluate_h_with(inp, None, None, values)
}

/// `try_evaluate_h` with the shuffle stage after the lookups (`h2hip_evaluate_h_shuffles_bn254`)
pub fn try_evaluate_h_shuffles<F: 'static + Copy>(inp: &EvalHInput<'_, F>, shuffles: &ShufflesInput<'_, F>, values: &mut [F]) -> bool {
    evaluate_h_with(inp, None, Some(shuffles), values)
}

/// `try_evaluate_h` with every argument that travels beside the description (`h2hip_evaluate_h_ext_bn254`): the mv-lookup stage after
/// the halo2 lookups, then the shuffle stage; either may be absent
pub fn try_evaluate_h_ext<F: 'static + Copy>(inp: &EvalHInput<'_, F>, mvlookups: Option<&MvLookupsInput<'_, F>>,
                                             shuffles: Option<&ShufflesInput<'_, F>>, values: &mut [F]) -> bool {
    evaluate_h_with(inp, mvlookups, shuffles, values)
}

fn evaluate_h_with<F: 'static + Copy>(inp: &EvalHInput<'_, F>, mvlookups: Option<&MvLookupsInput<'_, F>>,
                                      shuffles: Option<&ShufflesInput<'_, F>>, values: &mut [F]) -> bool {
    if std::any::TypeId::of::<F>() != std::any::TypeId::of::<halo2curves::bn256::Fr>() || std::mem::size_of::<F>() != 32 {
        return false;
    }
    let n = 1usize << inp.k;
    let en = 1usize << inp.extended_k;
    let all_len = |v: &Vec<&[F]>, len: usize| v.iter().all(|s| s.len() == len);
    let n_lookups = inp.lookup_graphs.len();
    if values.len() != en
        || !all_len(&inp.fixed_cosets, en)
        || !all_len(&inp.advice_polys, n)
        || !all_len(&inp.instance_polys, n)
        || inp.l0.len() != en
        || inp.l_last.len() != en
        || inp.l_active_row.len() != en
        || !all_len(&inp.perm_product_cosets, en)
        || !all_len(&inp.perm_cosets, en)
        || inp.perm_cosets.len() != inp.perm_columns.len()
        || !all_len(&inp.lookup_product_polys, n)
        || !all_len(&inp.lookup_permuted_input_polys, n)
        || !all_len(&inp.lookup_permuted_table_polys, n)
        || inp.lookup_product_polys.len() != n_lookups
        || inp.lookup_permuted_input_polys.len() != n_lookups
        || inp.lookup_permuted_table_polys.len() != n_lookups
    {
        return false;
    }
    let table = |v: &Vec<&[F]>| -> Vec<*const u64> { v.iter().map(|s| s.as_ptr() as *const u64).collect() };
    let fixed = table(&inp.fixed_cosets);
    let advice = table(&inp.advice_polys);
    let instance = table(&inp.instance_polys);
    let perm_prod = table(&inp.perm_product_cosets);
    let perm_cosets = table(&inp.perm_cosets);
    let lk_prod = table(&inp.lookup_product_polys);
    let lk_in = table(&inp.lookup_permuted_input_polys);
    let lk_tab = table(&inp.lookup_permuted_table_polys);
    let kinds: Vec<u32> = inp.perm_columns.iter().map(|c| c.0).collect();
    let indices: Vec<u32> = inp.perm_columns.iter().map(|c| c.1).collect();
    let lookup_views: Vec<h2hip_graph> = inp.lookup_graphs.iter().map(|g| g.view()).collect();
    let p = |x: &F| x as *const F as *const u64;
    let desc = h2hip_evalh_desc {
        k: inp.k,
        extended_k: inp.extended_k,
        extended_omega: p(&inp.extended_omega),
        g_coset: p(&inp.g_coset),
        g_coset_inv: p(&inp.g_coset_inv),
        n_fixed: fixed.len() as u32,
        n_advice: advice.len() as u32,
        n_instance: instance.len() as u32,
        n_challenges: inp.challenges.len() as u32,
        fixed_cosets: fixed.as_ptr(),
        advice_polys: advice.as_ptr(),
        instance_polys: instance.as_ptr(),
        challenges: inp.challenges.as_ptr() as *const u64,
        y: p(&inp.y),
        beta: p(&inp.beta),
        gamma: p(&inp.gamma),
        theta: p(&inp.theta),
        l0: inp.l0.as_ptr() as *const u64,
        l_last: inp.l_last.as_ptr() as *const u64,
        l_active_row: inp.l_active_row.as_ptr() as *const u64,
        custom_gates: inp.custom_gates.view(),
        n_perm_sets: perm_prod.len() as u32,
        n_perm_columns: perm_cosets.len() as u32,
        chunk_len: inp.chunk_len,
        last_rotation: inp.last_rotation,
        perm_product_cosets: perm_prod.as_ptr(),
        perm_column_kind: kinds.as_ptr(),
        perm_column_index: indices.as_ptr(),
        perm_cosets: perm_cosets.as_ptr(),
        zeta: p(&inp.zeta),
        delta: p(&inp.delta),
        n_lookups: n_lookups as u32,
        lookup_graphs: lookup_views.as_ptr(),
        lookup_product_polys: lk_prod.as_ptr(),
        lookup_permuted_input_polys: lk_in.as_ptr(),
        lookup_permuted_table_polys: lk_tab.as_ptr(),
    };
    // The proving key's own columns -- pk.fixed_cosets, pk.l0 / l_last / l_active_row, pk.permutation.cosets -- do not change from proof to
    // proof: keep them in HBM across calls (idempotent; fingerprint-guarded like the pinned bases; a failure only means they are uploaded
    // per call).  `unpin_key_columns` in ProvingKey's Drop (patch 0006) releases them.
    let mut key_columns: Vec<*const u64> = fixed.clone();
    key_columns.extend_from_slice(&perm_cosets);
    key_columns.push(desc.l0);
    key_columns.push(desc.l_last);
    key_columns.push(desc.l_active_row);
    let _ = unsafe { super::ffi::h2hip_columns_pin(key_columns.as_ptr(), key_columns.len(), en) };
    // the extras' tables live until the call returns; an absent extra is a null struct pointer
    let sh_tabs = match shuffles.map(|sh| shuffles_view(sh, n)) {
        Some(None) => return false,
        Some(v) => v,
        None => None,
    };
    let mv_tabs = match mvlookups.map(|mv| mvlookups_view(mv, n)) {
        Some(None) => return false,
        Some(v) => v,
        None => None,
    };
    let c_sh = sh_tabs.as_ref().map(|(views, polys)| EvalhShuffles { n_shuffles: polys.len() as u32, graphs: views.as_ptr(), product_polys: polys.as_ptr() });
    let c_mv = match (mvlookups, mv_tabs.as_ref()) {
        (Some(mv), Some((views, phi, m))) => Some(EvalhMvLookups {
            n_args: mv.n_inputs.len() as u32,
            n_inputs: mv.n_inputs.as_ptr(),
            graphs: views.as_ptr(),
            phi_polys: phi.as_ptr(),
            m_polys: m.as_ptr(),
        }),
        _ => None,
    };
    if c_mv.is_none() && c_sh.is_none() {
        return unsafe { super::ffi::h2hip_evaluate_h_bn254(&desc as *const h2hip_evalh_desc, values.as_mut_ptr() as *mut u64) } == 0;
    }
    let rc: c_int = unsafe {
        super::ffi::h2hip_evaluate_h_ext_bn254(&desc as *const h2hip_evalh_desc, c_mv.as_ref().map_or(std::ptr::null(), |c| c as *const EvalhMvLookups),
                                               c_sh.as_ref().map_or(std::ptr::null(), |c| c as *const EvalhShuffles), values.as_mut_ptr() as *mut u64)
    };
    rc == 0
}

/// Release the device copies `try_evaluate_h` keeps of a proving key's constant columns (call from `ProvingKey`'s `Drop`, before the
/// `Vec`s are freed; unknown pointers are ignored, other element types are a no-op).
pub fn unpin_key_columns<F: 'static>(columns: &[&[F]]) {
    if std::any::TypeId::of::<F>() != std::any::TypeId::of::<halo2curves::bn256::Fr>() || columns.is_empty() {
        return;
    }
    let ptrs: Vec<*const u64> = columns.iter().map(|c| c.as_ptr() as *const u64).collect();
    unsafe { super::ffi::h2hip_columns_unpin(ptrs.as_ptr(), ptrs.len()) };
}

/// One circuit instance of `evaluate_h` evaluated one coset of the 2^k domain at a time: `EvalHInput` with every column a polynomial in
/// coefficient form (2^k each), so that neither the proving key nor the engine holds an extended coset.
pub struct EvalHPartsInput<'a, F> {
    pub k: u32,
    pub extended_k: u32,
    pub extended_omega: F,
    pub g_coset: F,
    pub g_coset_inv: F,
    /// pk.fixed_polys
    pub fixed_polys: Vec<&'a [F]>,
    pub advice_polys: Vec<&'a [F]>,
    pub instance_polys: Vec<&'a [F]>,
    pub challenges: &'a [F],
    pub y: F,
    pub beta: F,
    pub gamma: F,
    pub theta: F,
    /// pk.l0 / l_last / l_active_row as polynomials
    pub l0_poly: &'a [F],
    pub l_last_poly: &'a [F],
    pub l_active_row_poly: &'a [F],
    pub custom_gates: &'a FlatGraph,
    /// sets[i].permutation_product_poly; empty skips the permutation argument
    pub perm_product_polys: Vec<&'a [F]>,
    pub perm_columns: Vec<(u32, u32)>,
    /// pk.permutation.polys[j]
    pub perm_polys: Vec<&'a [F]>,
    pub chunk_len: u32,
    pub last_rotation: i32,
    pub zeta: F,
    pub delta: F,
    pub lookup_graphs: &'a [FlatGraph],
    pub lookup_product_polys: Vec<&'a [F]>,
    pub lookup_permuted_input_polys: Vec<&'a [F]>,
    pub lookup_permuted_table_polys: Vec<&'a [F]>,
    /// the parts this call computes, `part_begin .. part_begin + part_count` of the 2^(extended_k - k); 0, 0 = all of them
    pub part_begin: u32,
    pub part_count: u32,
    /// `EvaluationDomain::t_evaluations` on the call of the last circuit instance: `values` then leaves as
    /// `divide_by_vanishing_poly(h)`; `None` otherwise
    pub t_evaluations: Option<&'a [F]>,
}

/// Safe front of `h2hip_evaluate_h_parts_bn254`: checks the element type and every slice length, builds the pointer tables, calls the
/// engine.  `values` (2^extended_k elements) is read and written on the rows of the requested parts only.  false: the engine declined,
/// run the CPU body.
pub fn try_evaluate_h_parts<F: 'static + Copy>(inp: &EvalHPartsInput<'_, F>, values: &mut [F]) -> bool {
    evaluate_h_parts_with(inp, None, None, values)
}

/// `try_evaluate_h_parts` with the shuffle stage after the lookups (`h2hip_evaluate_h_parts_shuffles_bn254`)
pub fn try_evaluate_h_parts_shuffles<F: 'static + Copy>(inp: &EvalHPartsInput<'_, F>, shuffles: &ShufflesInput<'_, F>, values: &mut [F]) -> bool {
    evaluate_h_parts_with(inp, None, Some(shuffles), values)
}

/// `try_evaluate_h_parts` with every argument that travels beside the description (`h2hip_evaluate_h_parts_ext_bn254`)
pub fn try_evaluate_h_parts_ext<F: 'static + Copy>(inp: &EvalHPartsInput<'_, F>, mvlookups: Option<&MvLookupsInput<'_, F>>,
                                                   shuffles: Option<&ShufflesInput<'_, F>>, values: &mut [F]) -> bool {
    evaluate_h_parts_with(inp, mvlookups, shuffles, values)
}

fn evaluate_h_parts_with<F: 'static + Copy>(inp: &EvalHPartsInput<'_, F>, mvlookups: Option<&MvLookupsInput<'_, F>>,
                                            shuffles: Option<&ShufflesInput<'_, F>>, values: &mut [F]) -> bool {
    if std::any::TypeId::of::<F>() != std::any::TypeId::of::<halo2curves::bn256::Fr>() || std::mem::size_of::<F>() != 32 {
        return false;
    }
    if inp.extended_k < inp.k || inp.extended_k > 28 {
        return false;
    }
    let n = 1usize << inp.k;
    let en = 1usize << inp.extended_k;
    let all_n = |v: &Vec<&[F]>| v.iter().all(|s| s.len() == n);
    let n_lookups = inp.lookup_graphs.len();
    if values.len() != en
        || !all_n(&inp.fixed_polys)
        || !all_n(&inp.advice_polys)
        || !all_n(&inp.instance_polys)
        || inp.l0_poly.len() != n
        || inp.l_last_poly.len() != n
        || inp.l_active_row_poly.len() != n
        || !all_n(&inp.perm_product_polys)
        || !all_n(&inp.perm_polys)
        || inp.perm_polys.len() != inp.perm_columns.len()
        || !all_n(&inp.lookup_product_polys)
        || !all_n(&inp.lookup_permuted_input_polys)
        || !all_n(&inp.lookup_permuted_table_polys)
        || inp.lookup_product_polys.len() != n_lookups
        || inp.lookup_permuted_input_polys.len() != n_lookups
        || inp.lookup_permuted_table_polys.len() != n_lookups
        || inp.t_evaluations.map_or(false, |t| t.len() != en / n)
    {
        return false;
    }
    let table = |v: &Vec<&[F]>| -> Vec<*const u64> { v.iter().map(|s| s.as_ptr() as *const u64).collect() };
    let fixed = table(&inp.fixed_polys);
    let advice = table(&inp.advice_polys);
    let instance = table(&inp.instance_polys);
    let perm_prod = table(&inp.perm_product_polys);
    let perm_polys = table(&inp.perm_polys);
    let lk_prod = table(&inp.lookup_product_polys);
    let lk_in = table(&inp.lookup_permuted_input_polys);
    let lk_tab = table(&inp.lookup_permuted_table_polys);
    let kinds: Vec<u32> = inp.perm_columns.iter().map(|c| c.0).collect();
    let indices: Vec<u32> = inp.perm_columns.iter().map(|c| c.1).collect();
    let lookup_views: Vec<h2hip_graph> = inp.lookup_graphs.iter().map(|g| g.view()).collect();
    let p = |x: &F| x as *const F as *const u64;
    let desc = EvalhPartsDesc {
        k: inp.k,
        extended_k: inp.extended_k,
        extended_omega: p(&inp.extended_omega),
        g_coset: p(&inp.g_coset),
        g_coset_inv: p(&inp.g_coset_inv),
        n_fixed: fixed.len() as u32,
        n_advice: advice.len() as u32,
        n_instance: instance.len() as u32,
        n_challenges: inp.challenges.len() as u32,
        fixed_polys: fixed.as_ptr(),
        advice_polys: advice.as_ptr(),
        instance_polys: instance.as_ptr(),
        challenges: inp.challenges.as_ptr() as *const u64,
        y: p(&inp.y),
        beta: p(&inp.beta),
        gamma: p(&inp.gamma),
        theta: p(&inp.theta),
        l0_poly: inp.l0_poly.as_ptr() as *const u64,
        l_last_poly: inp.l_last_poly.as_ptr() as *const u64,
        l_active_row_poly: inp.l_active_row_poly.as_ptr() as *const u64,
        custom_gates: inp.custom_gates.view(),
        n_perm_sets: perm_prod.len() as u32,
        n_perm_columns: perm_polys.len() as u32,
        chunk_len: inp.chunk_len,
        last_rotation: inp.last_rotation,
        perm_product_polys: perm_prod.as_ptr(),
        perm_column_kind: kinds.as_ptr(),
        perm_column_index: indices.as_ptr(),
        perm_polys: perm_polys.as_ptr(),
        zeta: p(&inp.zeta),
        delta: p(&inp.delta),
        n_lookups: n_lookups as u32,
        lookup_graphs: lookup_views.as_ptr(),
        lookup_product_polys: lk_prod.as_ptr(),
        lookup_permuted_input_polys: lk_in.as_ptr(),
        lookup_permuted_table_polys: lk_tab.as_ptr(),
        part_begin: inp.part_begin,
        part_count: inp.part_count,
        t_evaluations: inp.t_evaluations.map_or(std::ptr::null(), |t| t.as_ptr() as *const u64),
    };
    let sh_tabs = match shuffles.map(|sh| shuffles_view(sh, n)) {
        Some(None) => return false,
        Some(v) => v,
        None => None,
    };
    let mv_tabs = match mvlookups.map(|mv| mvlookups_view(mv, n)) {
        Some(None) => return false,
        Some(v) => v,
        None => None,
    };
    let c_sh = sh_tabs.as_ref().map(|(views, polys)| EvalhShuffles { n_shuffles: polys.len() as u32, graphs: views.as_ptr(), product_polys: polys.as_ptr() });
    let c_mv = match (mvlookups, mv_tabs.as_ref()) {
        (Some(mv), Some((views, phi, m))) => Some(EvalhMvLookups {
            n_args: mv.n_inputs.len() as u32,
            n_inputs: mv.n_inputs.as_ptr(),
            graphs: views.as_ptr(),
            phi_polys: phi.as_ptr(),
            m_polys: m.as_ptr(),
        }),
        _ => None,
    };
    if c_mv.is_none() && c_sh.is_none() {
        return unsafe { super::ffi::h2hip_evaluate_h_parts_bn254(&desc as *const EvalhPartsDesc, values.as_mut_ptr() as *mut u64) } == 0;
    }
    let rc: c_int = unsafe {
        super::ffi::h2hip_evaluate_h_parts_ext_bn254(&desc as *const EvalhPartsDesc, c_mv.as_ref().map_or(std::ptr::null(), |c| c as *const EvalhMvLookups),
                                                     c_sh.as_ref().map_or(std::ptr::null(), |c| c as *const EvalhShuffles), values.as_mut_ptr() as *mut u64)
    };
    rc == 0
}
