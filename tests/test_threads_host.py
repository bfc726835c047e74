"""gsr_last_error() per host thread, without a GPU.

The message buffer is `thread_local` (csrc/gsr_common.hip: g_err): a thread reads the message of ITS last failed call, whatever another
thread failed at in between.  The two refusals used here are the first statement of their entry, in front of any HIP call
(csrc/gsr_densify.hip: gsr_gather_rows refuses more than 16 groups, gsr_split_children a scale_dims other than 2 or 3), so nothing is
launched and no device is needed."""
import thread_probe as TP


def test_last_error_is_the_calling_threads_own(hip_lib_built):
    import _gsr
    lib = _gsr.lib
    bar = TP.Barrier(2, timeout_s=30.0)
    groups = (_gsr.GatherGroup * 17)()

    def fail_a():
        return lib.gsr_gather_rows(None, None, None, 4, groups, 17, None)

    def fail_b():
        return lib.gsr_split_children(1, 5, 2, None, None, None, None, None, None, None, None)

    def worker(fail, first):
        def fn():
            mine_before = lib.gsr_last_error()
            if not first:
                bar.wait("A has failed")
            rc = fail()
            if first:
                bar.wait("A has failed")
            bar.wait("B has failed")
            if not first:
                bar.wait("A has read")
            msg = lib.gsr_last_error()
            if first:
                bar.wait("A has read")
            return rc, mine_before, msg
        return fn
    # A fails, barrier, B fails, barrier, A reads, barrier, B reads
    (rc_a, before_a, msg_a), (rc_b, before_b, msg_b) = TP.run_threads([worker(fail_a, True), worker(fail_b, False)], names=["A", "B"],
                                                                      rendezvous=[bar])
    assert rc_a < 0 and rc_b < 0
    assert before_a == b"" and before_b == b"", "a fresh thread starts with an empty message"
    assert b"gsr_gather_rows: at most 16 groups" in msg_a, msg_a
    assert b"gsr_split_children: invalid argument" in msg_b, msg_b
    # and the main thread, which failed at neither, sees neither
    main = lib.gsr_last_error()
    assert b"at most 16 groups" not in main and b"gsr_split_children" not in main
