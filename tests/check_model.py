"""A plain-Python transcription of one request's Check, written from the Go:

  dispatcher.Check      mixer/pkg/runtime/dispatcher.go:216-236 (dispatch :175-183 issues one call per
                        (action, instance) in order; safeDispatch turns a panic into res == nil, err != nil)
  combineResults        dispatcher.go:322-361, CheckResult.Combine mixer/pkg/adapter/check.go:45-57
  grpcServer.Check      mixer/pkg/api/grpcServer.go:160-179 (checkOk: 10 s / 200, :56-65)
  HandleListEntry       mixer/adapter/list/list.go:68-101; listentry ProcessCheck
                        mixer/template/template.gen.go:2153-2202

The reference collects the calls' results in completion order (dispatcher.go:392-394); the model,
like the product, takes them in the order they are issued -- one of the orders the reference can
produce.

Inputs per request: the Resolve status (0 = resolved), the selected rules in order, rule -> units,
and per unit what its call returned:  (code, valid_duration_ns, valid_use_count, value)  with code
the google.rpc code (const units: their configured one), EVAL_ERROR (-1: Value's Eval failed) or
NOT_STRING (-2: the type assertion panicked); value is the Value register of a failing list unit,
0 otherwise.  Outputs: the result tuple and the records."""

OK, INTERNAL = 0, 13
EVAL_ERROR, NOT_STRING = -1, -2
F_RESOLVE_ERROR, F_NO_CHECKS, F_EVAL_ERROR, F_UNIT_PANIC = 1, 2, 4, 8
DEFAULTS = (10 * 10 ** 9, 200)  # checkOk (grpcServer.go:56-65)


def check_request(status, rules, rule_units, unit_result, defaults=DEFAULTS):
    """-> ((valid_duration_ns, valid_use_count, code, n_records, flags), records) with records a list of
    (rule, unit, code, value), one per unit whose code is not OK, in dispatch order.

    rule_units[r]: rule r's unit indices in configuration order; unit_result(u) -> (code, duration,
    use count, value) of unit u for this request."""
    if status != 0:
        # Resolve failed: dispatcher.Check returns (nil, err) (dispatcher.go:218-221); grpcServer:
        # out = status.WithError(err), cr == nil -> checkOk's numbers
        return (defaults[0], defaults[1], INTERNAL, 0, F_RESOLVE_ERROR), []
    res = None          # combineResults' `res` (the first non-nil result, combined in place)
    err = False         # ... and its multierror
    code, failed = OK, False
    flags, records = 0, []
    for r in rules:                 # dispatch: actions in order ...
        for u in rule_units[r]:     # ... and each action's instances in order
            c, dur, use, value = unit_result(u)
            if c != OK:
                records.append((r, u, c, value if c > 0 else 0))
            if c == NOT_STRING:
                # panic: safeDispatch -> result{err: ...}, res nil: `continue` (dispatcher.go:332-334)
                err = True
                flags |= F_UNIT_PANIC
                continue
            if c == EVAL_ERROR:
                # ProcessCheck: `return adapter.CheckResult{}, err`; dispatcher.go:227 stores &res:
                # a zero result takes part
                err = True
                flags |= F_EVAL_ERROR
                c, dur, use = OK, 0, 0
            if res is None:
                res = [dur, use]
            else:                   # CheckResult.Combine
                if res[0] > dur:
                    res[0] = dur
                if res[1] > use:
                    res[1] = use
            if c != OK and not failed:  # "the first failure result's code becomes the result code"
                code, failed = c, True
    if res is None:
        # cr == nil -> checkOk; out stays OK unless err != nil (status.WithError: INTERNAL)
        return (defaults[0], defaults[1], INTERNAL if err else OK, len(records), flags | F_NO_CHECKS), records
    # cr != nil: out = cr.Status, whatever err says (grpcServer.go:168-170)
    return (res[0], res[1], code, len(records), flags), records


def message(records, handler_name, unit_message):
    """combineResults' text (dispatcher.go:344-352): "<handler>:<message>" of every failed result,
    joined by ", ".  handler_name(u) -> str; unit_message(u, code, value) -> str."""
    return ", ".join("%s:%s" % (handler_name(u), unit_message(u, c, v)) for _, u, c, v in records if c > 0)


def list_message(code, symbol):
    """HandleListEntry's status message (list.go:80-93; the IP list's error text ipList.go:77-92)"""
    return {5: "%s is not whitelisted", 7: "%s is blacklisted", 3: "%s is not a valid IP address"}[code] % symbol
